"""``ops.gemm.report()`` returns the whole plan table.  The planner fills what fits into the
caller's buffer; a process that had tuned a few hundred GEMM shapes got a table cut at 64 KiB, and
the keys that sort last were missing from it."""
import ctypes

from distributed_llm_trainer_amd.ops import gemm


class _FakePlanner:
    """dlt_gemm_report of csrc_gemm/gemm_planner.cpp on a fixed table: copies min(size, len - 1)."""

    def __init__(self, table: bytes):
        self.table, self.calls = table, []

    def dlt_gemm_report(self, buf, length):
        self.calls.append(length)
        n = min(len(self.table), length - 1)
        ctypes.memmove(buf, self.table, n)
        buf[n] = b"\0"
        return n


def _table(lines: int) -> str:
    return "".join(f"ta=1 tb=0 m={640 + i} n=768 k=384 acc=0 dtc=1 cand=8 chosen=-1 sol={i} us=12.5 kernel_{i}\n"
                   for i in range(lines))


def test_report_returns_a_table_larger_than_its_first_buffer(monkeypatch):
    want = _table(3000)
    assert len(want) > 3 * (1 << 16)
    fake = _FakePlanner(want.encode())
    monkeypatch.setattr(gemm, "lib", lambda: fake)
    got = gemm.report()
    assert got == want and got.splitlines()[-1].startswith("ta=1 tb=0 m=3639 ")
    assert len(fake.calls) > 1 and fake.calls[0] == 1 << 16


def test_report_of_a_small_table_takes_one_call(monkeypatch):
    want = _table(5)
    fake = _FakePlanner(want.encode())
    monkeypatch.setattr(gemm, "lib", lambda: fake)
    assert gemm.report() == want and fake.calls == [1 << 16]
