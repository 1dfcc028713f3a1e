"""CPU: the table of tests/fused_ln_cases.py against the C library's `mavlm_linear_ln_ws_bytes` - the function the operator asks
whether a shape runs as the fused dense + residual + LayerNorm kernel - under the hook each case sets; what the table covers; and
the planted residual pattern of `gpu_util.fused_ln_pattern` on the rows of every case.  No kernel is launched."""
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
import fused_ln_cases as F
from gpu_util import FUSED_LN_DISTANCES, FUSED_LN_UNIT, fused_ln_inputs, fused_ln_pattern


@pytest.fixture
def hook():
    """sets `mavlm_set_fused_layernorm`; the product's value (1) is back afterwards"""
    lib = capi.lib()

    def set_hook(v):
        capi.check(lib.mavlm_set_fused_layernorm(v), "hook")
    yield set_hook
    lib.mavlm_set_fused_layernorm(1)


def test_every_case_takes_the_fused_form(hook):
    ws = capi.lib().mavlm_linear_ln_ws_bytes
    for case in F.CASES:
        M, N, K, mode, fused, tile, rows, eps = case
        partners, want_hook, min_m = F.WIDTHS[N]
        assert fused == want_hook and partners == N // 256 and M >= min_m, case
        assert tile in (0, 129) and rows in F.HEIGHTS and mode in ("bf16", "fp16") and K % 64 == 0, case
        hook(fused)
        assert ws(M, N, K) > 0, case
        # the scratch the kernel indexes: [row blocks][partners][256 rows (128 in gemm128.hip)][2] 8-byte granules behind 64 bytes
        # of control words
        height, slots = (128, 128) if tile == 129 else (rows, 256)
        assert ws(M, N, K) >= 64 + -(-M // height) * partners * slots * 2 * 8, case
        hook(1)
        assert (ws(M, N, K) > 0) == (N <= 1024), case           # the product's rule stops at 4 partners
        hook(0)
        assert ws(M, N, K) == 0, case


def test_the_smallest_rows_are_the_smallest(hook):
    ws = capi.lib().mavlm_linear_ln_ws_bytes
    for N, (partners, fused, min_m) in F.WIDTHS.items():
        hook(fused)
        assert (min_m - 1) % 256 == 0 and -(-min_m // 256) * partners >= 192 > (min_m - 1) // 256 * partners
        for K in (64, 192, 1024):
            assert ws(min_m, N, K) > 0 and ws(min_m - 1, N, K) == 0, (N, K)       # one row block fewer: the two-kernel form
        assert ws(min_m, N, 96) == 0 and ws(min_m, N + 128, 64) == 0
    hook(2)
    assert capi.lib().mavlm_linear_ln_ws_bytes(2817 * 2, 4096 + 256, 64) == 0          # 17 partners: never


def test_what_the_table_covers():
    cases = F.CASES
    assert 40 <= len(cases) <= 48 and len(set(cases)) == len(cases)
    assert {N // 256 for _, N, *_ in cases} == set(F.PARTNERS) == {p for p, _, _ in F.WIDTHS.values()}
    plain = [c for c in cases if c[5] == 0]
    for h in F.HEIGHTS:
        assert {0, 1, h - 1} <= {M % h for M, N, K, mode, fused, tile, rows, eps in plain if rows == h and N == 1024}, h
        for N in F.WIDTHS:                                      # every width: a ragged last row block at each height, both types
            assert any(M % h for M, n, K, mode, fused, tile, rows, eps in plain if rows == h and n == N), (N, h)
            assert {c[3] for c in plain if c[1] == N} == {"bf16", "fp16"}, N
        # a last row block of ONE valid row (its other rows are clamped to row M - 1)
        assert any(M % h == 1 for M, N, K, mode, fused, tile, rows, eps in plain if rows == h)
        assert any(-(-M // h) * (N // 256) > 256 for M, N, K, mode, fused, tile, rows, eps in plain if rows == h), h
    assert {64, 192, 1024} <= {K for _, _, K, *_ in cases}
    assert {eps for *_, eps in cases} == {1e-12, 1e-5}
    for mode in ("bf16", "fp16"):
        assert any(c[3] == mode and c[7] == 1e-5 for c in cases) and any(c[3] == mode and c[2] == 64 for c in cases)
    t129 = [c for c in cases if c[5] == 129]
    assert len(t129) == 3 and {c[3] for c in t129} == {"bf16", "fp16"} and len({c[1] for c in t129}) >= 2
    for M, N, K, mode, fused, tile, rows, eps in t129:          # each is one of the 256-row cases, and ragged at 128 rows
        assert any(c[:4] == (M, N, K, mode) and c[5] == 0 and c[7] == eps for c in cases) and M % 128 in (1, 127)


def test_planted_rows_differ_at_every_distance_of_the_epilogue():
    """Rows r and r + d, d = 1 (the neighbour), 16 (the MFMA row fragment), 112 / 128 (half a tile of 224 / 256 rows, and the tile
    of gemm128.hip), 224 / 256 (the tile): different scales, or at least one tile offset apart by a unit or more - for every row of
    every (M, N) of the table.  A row normalised with the statistics of such a neighbour cannot come out right."""
    assert set(FUSED_LN_DISTANCES) == {1, 16, 112, 128, 224, 256}
    for M, N in sorted({(c[0], c[1]) for c in F.CASES}):
        s, o = fused_ln_pattern(M, N // 256)
        assert s.shape == (M,) and o.shape == (M, N // 256)
        assert int(s.min()) == 0 and int(s.max()) == 4 and int(o.min()) == 0 and int(o.max()) == 16
        for d in FUSED_LN_DISTANCES:
            differ = (s[:-d] != s[d:]) | ((o[:-d] - o[d:]).abs() >= 1).any(dim=1)
            assert bool(differ.all()), (M, N, d, int((~differ).nonzero()[0]))
        if N > 256:                                             # and the tiles of a row all differ from one another
            srt = o.sort(dim=1).values
            assert bool((srt[:, 1:] > srt[:, :-1]).all()), (M, N)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_planted_residual_is_the_pattern(mode):
    """`fused_ln_inputs`: the planted residual minus the plain one (same seed) is the pattern - scale s(r), offsets of whole units of
    several sigma, all exact on the 16-bit grid -, and the other operands do not depend on `planted`."""
    M, N, K = 300, 768, 64
    a = fused_ln_inputs(M, N, K, mode, 5, planted=True, device="cpu")
    p = fused_ln_inputs(M, N, K, mode, 5, planted=False, device="cpu")
    for i in (0, 1, 2, 4, 5):
        assert torch.equal(a[i], p[i])
    assert a[3].dtype == a[0].dtype == a[1].dtype and a[2].dtype == a[4].dtype == a[5].dtype == torch.float32
    s, o = fused_ln_pattern(M, N // 256)
    scale = torch.exp2((s - 2).double())[:, None]
    off = ((o - 8).double() * FUSED_LN_UNIT).repeat_interleave(256, dim=1)
    assert float(off.abs().max()) == 4.0 and torch.equal(off.to(a[3].dtype).double(), off)
    tile_mean = (a[3].double() / scale).view(M, N // 256, 256).mean(dim=2)
    assert float((tile_mean - (o - 8).double() * FUSED_LN_UNIT).abs().max()) < 0.3            # N(0,1) / 16 = 0.06 per tile mean
    assert float((a[3].double() / scale - off - p[3].double()).abs().max()) <= 2.0 ** -5    # one rounding of values below 16
