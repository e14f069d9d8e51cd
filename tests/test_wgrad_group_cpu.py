"""Share apportioning and workgroup placement of the grouped weight gradient
(ops/hip.py wgrad_group_shares / wgrad_group_table): pure arithmetic, no GPU."""
import pytest

from distributed_llm_trainer_amd.ops import hip

SMALL = ((768, 3072), (6144, 768), (768, 768), (2304, 768))  # down, gate/up, o, qkv of the small preset
GROUPS = [(32768, SMALL, 256), (32768, SMALL, 224), (32768, SMALL, 192),
          (32768, (SMALL[0], SMALL[2], SMALL[3]), 256),
          (1024, ((256, 192), (768, 384), (384, 192), (512, 768)), 256),
          (2048, ((256, 192), (768, 384), (384, 192), (512, 768)), 256),
          (1024, ((384, 1536), (3072, 384), (384, 384), (1152, 384)), 256),
          (16384, ((1024, 4096), (8192, 1024), (1024, 1024), (3072, 1024)), 256)]


def _ntc(shapes):
    return [nc // hip.wgrad_bn(nc) for _, nc in shapes]


@pytest.mark.parametrize("T,shapes,grid", GROUPS)
def test_shares_fit_the_grid(T, shapes, grid):
    shares = hip.wgrad_group_shares(T, shapes, grid)
    assert len(shares) == len(shapes) and all(s >= 1 for s in shares)
    assert sum(s * c for s, c in zip(shares, _ntc(shapes))) <= grid
    # a share is at least one (row tile, token pair) iteration
    assert all(s <= ((nr + 255) // 256) * (T // 128) for s, (nr, _) in zip(shares, shapes))


def test_small_preset_split():
    shares = hip.wgrad_group_shares(32768, SMALL)
    assert shares == [4, 32, 4, 12]
    pairs = [((nr + 255) // 256) * (32768 // 128) / s for s, (nr, _) in zip(shares, SMALL)]
    assert pairs == [192.0] * 4
    assert hip.wgrad_group_shares(32768, (SMALL[0], SMALL[2], SMALL[3])) == [8, 8, 24]  # 96 pairs each


@pytest.mark.parametrize("T,shapes,grid", GROUPS)
@pytest.mark.parametrize("spread", [False, True])
def test_table_places_every_workgroup_once(T, shapes, grid, spread):
    shares = hip.wgrad_group_shares(T, shapes, grid)
    table = hip.wgrad_group_table(shapes, shares, spread=spread)
    assert len(table) % 8 == 0
    work = [e for e in table if e is not None]
    want = {(p, c, g) for p, n in enumerate(_ntc(shapes)) for c in range(n) for g in range(shares[p])}
    assert len(work) == len(want) and set(work) == want
    # the column tiles of one share read the same dY rows: one XCD (ids equal mod 8)
    xcd = {}
    for i, e in enumerate(table):
        if e is not None:
            assert xcd.setdefault((e[0], e[2]), i % 8) == i % 8


@pytest.mark.parametrize("spread", [False, True])
def test_small_preset_xcds_are_even(spread):
    for shapes, grid in ((SMALL, 256), (SMALL, 192), ((SMALL[0], SMALL[2], SMALL[3]), 256)):
        table = hip.wgrad_group_table(shapes, hip.wgrad_group_shares(32768, shapes, grid), spread=spread)
        assert len(table) == grid and None not in table
        assert [sum(1 for i, e in enumerate(table) if i % 8 == x) for x in range(8)] == [grid // 8] * 8


def test_small_preset_packing():
    """256 workgroups: two 16-column down shares fill an XCD, the four-column shares the
    other six; a problem's shares sit on as few XCDs as their number allows."""
    table = hip.wgrad_group_table(SMALL, [4, 32, 4, 12])
    xcds = [sorted({i % 8 for i, e in enumerate(table) if e[0] == p}) for p in range(4)]
    assert xcds == [[0, 1], [2, 3, 4, 5], [6], [6, 7]]
    # 192 workgroups (one whole tile each): shares [3, 24, 3, 9]
    assert hip.wgrad_group_shares(32768, SMALL, 192) == [3, 24, 3, 9]


@pytest.mark.parametrize("T,shapes,grid", GROUPS)
def test_xcd_counts_differ_by_less_than_one_share(T, shapes, grid):
    shares = hip.wgrad_group_shares(T, shapes, grid)
    table = hip.wgrad_group_table(shapes, shares, spread=True)
    counts = [sum(1 for i, e in enumerate(table) if e is not None and i % 8 == x) for x in range(8)]
    assert max(counts) - min(counts) <= max(_ntc(shapes))


def test_group_that_does_not_tile():
    with pytest.raises(ValueError):
        hip.wgrad_group_shares(1024, ((256, 192), (256, 128)))
    with pytest.raises(ValueError):
        hip.wgrad_group_shares(1024, ((64, 192),))
