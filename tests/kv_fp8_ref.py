"""The FP8 KV cache for tests: e4m3fn(clamp(x16, -448, 448)) (torch alone gives NaN above ~464), a guarded byte cache."""
import torch

FP8 = torch.float8_e4m3fn
NAN_BYTE = 0x7F  # e4m3fn's NaN: what the rows a kernel must not read are filled with
PAD = 64
# ties (17 -> 16, 19 -> 20, 2^-10 -> 0, 1.5 * 2^-9 -> 2^-8), 0, values beyond +-448, the smallest normal
PLANT = torch.tensor([17.0, 19.0, 2.0 ** -10, 1.5 * 2.0 ** -9, 0.0, 460.0, -1000.0, 2.0 ** -6])


def quant(x16: torch.Tensor) -> torch.Tensor:
    return x16.float().clamp(-448.0, 448.0).to(FP8).view(torch.uint8)


def planted(x: torch.Tensor) -> torch.Tensor:
    """``x`` cycling through saturating, ordinary and subnormal magnitudes; PLANT, then -0, open every row."""
    x = x * torch.tensor([600.0, 1.0, 2.0 ** -8, 30.0])[torch.arange(x.shape[-1]) % 4]
    x[..., :8], x[..., 8] = PLANT, -0.0
    return x


class Cache8:
    """A [B, nkv, maxS, hd] e4m3 cache ``t`` inside a larger byte allocation filled with ``fill``."""

    def __init__(self, shape, fill, device, init=None):
        n = int(torch.tensor(shape).prod())
        self.buf = torch.full((PAD + n + PAD,), fill, dtype=torch.uint8, device=device)
        self.u8 = self.buf[PAD:PAD + n].view(shape)
        if init is not None:
            self.u8.copy_(init)
        self.t = self.u8.view(FP8)
        assert self.t.data_ptr() % 16 == 0
        self.before = self.buf.clone()

    def assert_untouched(self, rows=None):
        # every byte outside the cache, and inside it every row but ``rows`` (a slice of dim 2), is as it was
        want = self.before.clone()
        if rows is not None:
            want[PAD:PAD + self.u8.numel()].view(self.u8.shape)[:, :, rows] = self.u8[:, :, rows]
        assert torch.equal(self.buf, want), "bytes outside the written rows changed"
