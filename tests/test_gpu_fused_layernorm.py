"""-m gpu: the fused dense + residual + LayerNorm GEMM (EPI_LN of csrc/gemm256.hip; csrc/gemm128.hip under `mavlm_set_gemm_tile(129)`)
against torch float64 on the GPU, gated per block of 4 rows x one 256-column tile.

The epilogue is where a row can go wrong on its own: a per-row reduction across four wave columns through LDS, per-tile (mean, M2)
published as {epoch, value} granules, the partners' granules polled into LDS, Chan's merge in tile order with the term 256 d^2
between tiles, the normalisation; rows past M are clamped to row M - 1.  tests/fused_ln_cases.py lists the launches - every
partner count 1, 2, 3, 4, 5, 8 and 16, tiles of 224 and 256 rows (128 in gemm128.hip) with M mod height = 0, 1 and height - 1, a
grid of more than one round of the chip, K = 64 (one K tile), 192 and 1024, bf16 and fp16, eps 1e-12 and 1e-5 - and
tests/test_fused_ln_cases_cpu.py holds that table to the C library without a GPU.

Inputs: `gpu_util.fused_ln_inputs`, planted - every row of the residual has its own scale and its own offset per column tile, so a
row normalised with another row's statistics, a tile's pair taken from another tile, a stale granule or a dropped between-tile
term cannot cancel (tests/test_gates_cpu.py plants each of these in ONE row of a restatement of the epilogue: >= 6.5 x floor; on
plain N(0,1) operands the first of them passes).  Reference: LayerNorm64(x.double() @ w.double().T + b + res), never another
kernel's output.  Gate: `gpu_util.fused_ln_gate`, BWD_BLOCK x the floor of the reference rounded once to the output grid; the
kernel computes in fp32 and rounds once, so the expected ratio is 1.0.  Measured ratios are printed (-s) and tabulated in
tests/README.md."""
import functools

import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from gpu_util import BWD_BLOCK, DT, LN_ROWS, fused_ln_gate, fused_ln_inputs, layernorm_ref64
import fused_ln_cases as F

pytestmark = pytest.mark.gpu
SENTINEL = -1234.0              # on both 16-bit grids; no operand and no output of these inputs comes near it
WORST = {}                      # (partners, height, mode) -> [worst block, whole tensor] x floor so far


@pytest.fixture
def hooks():
    """sets the three process-wide hooks of a case; the defaults are back afterwards, whatever happened"""
    lib = capi.lib()

    def set_hooks(fused, tile=0, rows=0):
        capi.check(lib.mavlm_set_fused_layernorm(fused), "fused layernorm")
        capi.check(lib.mavlm_set_gemm_tile(tile), "gemm tile")
        capi.check(lib.mavlm_set_gemm_rows(rows), "gemm rows")
    yield set_hooks
    lib.mavlm_set_fused_layernorm(1)
    lib.mavlm_set_gemm_tile(0)
    lib.mavlm_set_gemm_rows(0)


@functools.lru_cache(maxsize=4)
def _case(M, N, K, mode):
    """planted operands of a shape and the float64 z = x W^T + b, built once for the launches that share the shape"""
    args = fused_ln_inputs(M, N, K, mode, 7 * M + N + K)
    x, w, b = args[:3]
    return args, x.double() @ w.double().T + b.double()


def _ref64(args, pre64, eps):
    return layernorm_ref64(pre64, args[3], args[4], args[5], eps)


def _ctl():
    """(scratch, (arrivals, launch counter, timeout word)) of the operator's scratch on the current stream, after a sync"""
    ws = ops._LN_WS.get((torch.cuda.current_device(), ops.stream_ptr()))
    torch.cuda.synchronize()
    if ws is None:
        return None, (0, 0, 0)
    return ws, tuple(ws[:16].view(torch.int32)[:3].tolist())


def _launch(args, eps, want_pre=False, out=None):
    """one launch of the fused form with the control words checked around it: no arrival left behind, the launch counter advanced
    by exactly one, no timeout"""
    M, K = args[0].shape
    N = args[1].shape[0]
    assert capi.lib().mavlm_linear_ln_ws_bytes(M, N, K) > 0, "this shape does not take the fused form"
    ws0, before = _ctl()
    got, pre = ops.linear_residual_layernorm(*args, eps, want_pre=want_pre, out=out)
    ws1, after = _ctl()
    if ws1 is not ws0:                                          # a new, zero-filled scratch (first use or outgrown)
        before = (0, 0, 0)
    assert before[0] == 0 and before[2] == 0 and after == (0, before[1] + 1, 0), (before, after)
    return got, pre


def _gate(got, ref, mode, what, height):
    g = fused_ln_gate(got, ref, mode)
    rb, ct = g.where
    r0 = rb * LN_ROWS
    msg = (f"{what}: worst block {g.worst:.4f} x floor at rows {r0} .. {r0 + LN_ROWS - 1} (row block {rb} of {LN_ROWS} rows: tile row "
           f"{r0 // height}, row {r0 % height} of its {height}), column tile {ct}; whole tensor {g.whole:.4f} x floor "
           f"(floor {g.floor:.2e}, limit {BWD_BLOCK})")
    assert g.ok, msg
    assert g.whole <= BWD_BLOCK, msg
    return g, msg


@pytest.mark.parametrize("case", F.CASES, ids=[F.case_id(c) for c in F.CASES])
def test_fused_dense_residual_layernorm_vs_fp64(case, hooks):
    M, N, K, mode, fused, tile, rows, eps = case
    hooks(fused, tile, rows)
    height = 128 if tile == 129 else rows
    args, pre64 = _case(M, N, K, mode)
    out, pre = _launch(args, eps, want_pre=True)
    assert out.shape == (M, N) and out.dtype == DT[mode] and pre.shape == (M, N) and pre.dtype == torch.float32
    g, msg = _gate(out, _ref64(args, pre64, eps), mode, F.case_id(case), height)
    key = (N // 256, height, mode)
    WORST[key] = [max(a, b) for a, b in zip(WORST.get(key, [0.0, 0.0]), (g.worst, g.whole))]
    print(f"\n[fused-ln] {msg}\n[fused-ln-worst] partners {key[0]} height {key[1]} {key[2]}: {WORST[key][0]:.6f} {WORST[key][1]:.6f}")
    # the fp32 dense output (for the backward) is the plain GEMM's, bit for bit; a second launch repeats every bit
    assert torch.equal(pre, ops.linear(args[0], args[1], args[2], capi.EPI_F32))
    out2, pre2 = _launch(args, eps, want_pre=True)
    assert torch.equal(out2, out) and torch.equal(pre2, pre)
    if tile == 129:                                             # the 128-row form = the 256-row form on the planted rows
        hooks(fused, 0, 0)
        assert torch.equal(_launch(args, eps)[0], out)


@pytest.mark.parametrize("rows", F.HEIGHTS)
def test_strided_and_guarded_operands(rows, hooks):
    """x, res and out= are column slices of wider buffers filled with a sentinel (row strides of K + 16, N + 8 and N + 16 elements;
    res at the 8-byte alignment its loads need).  M = 12 289: one valid row in the last row block at 256 rows, 193 at 224.  Nothing
    outside [M, N] of the output buffer is written - its rows reach the end of the last 256-row tile -, the result passes the
    gate (a sentinel read as an operand would not), and `pre` has M rows."""
    M, N, K, mode, eps = 12289, 1024, 64, "bf16", 1e-12
    hooks(1, 0, rows)
    args, pre64 = _case(M, N, K, mode)
    x, w, b, res, gamma, beta = args
    xb = torch.full((M, K + 16), SENTINEL, device="cuda", dtype=DT[mode])
    rb = torch.full((M, N + 8), SENTINEL, device="cuda", dtype=DT[mode])
    ob = torch.full((-(-M // 256) * 256, N + 16), SENTINEL, device="cuda", dtype=DT[mode])
    xb[:, 8:8 + K], rb[:, 4:4 + N] = x, res
    xs, rs, os_ = xb[:, 8:8 + K], rb[:, 4:4 + N], ob[:M, 8:8 + N]
    assert xs.stride(0) == K + 16 and rs.stride(0) == N + 8 and os_.stride(0) == N + 16
    got, pre = _launch((xs, w, b, rs, gamma, beta), eps, want_pre=True, out=os_)
    assert got.data_ptr() == os_.data_ptr() and pre.shape == (M, N) and pre.is_contiguous()
    assert bool((ob[:, :8] == SENTINEL).all()) and bool((ob[:, 8 + N:] == SENTINEL).all()) and bool((ob[M:] == SENTINEL).all())
    _gate(os_, _ref64(args, pre64, eps), mode, f"strided operands, {rows}-row tiles", rows)
    assert torch.equal(os_, _launch(args, eps)[0])              # = the contiguous launch
    assert torch.equal(pre, ops.linear(x, w, b, capi.EPI_F32))


@pytest.mark.parametrize("M,N,fused", [(12289, 1024, 1), (16129, 768, 1), (9729, 1280, 2)], ids=["N1024", "N768", "N1280"])
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_constant_rows_give_beta_exactly(M, N, fused, mode, hooks):
    """x = 0, a constant bias and rows of `res` that are constant (values of few mantissa bits, another one in every row): every
    tile mean is the row's value exactly, every centred sum and every between-tile term is zero, the merged mean (a sum of 3, 4 or
    5 equal values divided by their count) is exact, and with eps = 1e-12 the output is beta, rounded - the fused counterpart of
    the constant-row check of the stand-alone kernel.  Both tile heights."""
    K, eps = 64, 1e-12
    _, w, _, _, gamma, beta = _case(M, N, K, mode)[0]
    x = torch.zeros((M, K), device="cuda", dtype=DT[mode])
    b = torch.full((N,), 0.75, device="cuda")
    values = torch.tensor([-3.0, -1.5, -0.5, 0.25, 1.0, 2.5, 6.0], device="cuda")
    res = values[torch.arange(M, device="cuda") * 5 % 7].to(DT[mode])[:, None].expand(M, N).contiguous()
    want = beta.to(DT[mode]).expand(M, N)
    for rows in F.HEIGHTS:
        hooks(fused, 0, rows)
        got, pre = _launch((x, w, b, res, gamma, beta), eps, want_pre=True)
        assert torch.equal(got, want), (rows, int((got != want).any(dim=1).nonzero()[0]))
        assert bool((pre == 0.75).all())


def test_scratch_shared_across_shapes(hooks):
    """One stream, one scratch: a shape with N = 1024, one with N = 512 (more row blocks, granules at other places, the epochs
    counting on), the first again.  Each launch is gated against float64; the third equals the first bit for bit."""
    hooks(1, 0, 256)
    eps = 1e-12
    a_args, a_pre64 = _case(12545, 1024, 64, "bf16")
    b_args, b_pre64 = _case(24321, 512, 64, "bf16")
    first = _launch(a_args, eps)[0]
    ws = _ctl()[0]
    _gate(first, _ref64(a_args, a_pre64, eps), "bf16", "N = 1024, first", 256)
    other = _launch(b_args, eps)[0]
    _gate(other, _ref64(b_args, b_pre64, eps), "bf16", "N = 512 on the scratch of N = 1024", 256)
    third = _launch(a_args, eps)[0]
    _gate(third, _ref64(a_args, a_pre64, eps), "bf16", "N = 1024 again", 256)
    assert _ctl()[0] is ws and torch.equal(third, first)


@pytest.mark.parametrize("M,N,K,mode", [(12545, 1024, 1024, "bf16"), (48897, 256, 64, "bf16"), (2817, 4096, 64, "fp16")],
                         ids=["N1024-bf16", "N256-bf16", "N4096-fp16"])
def test_two_kernel_form_passes_the_same_gate(M, N, K, mode, hooks):
    """`mavlm_set_fused_layernorm(0)`: the GEMM with its fp32 epilogue + the row LayerNorm kernel on the same planted operands pass
    the same gate - the gate is about the operation, not about one implementation."""
    hooks(0)
    assert capi.lib().mavlm_linear_ln_ws_bytes(M, N, K) == 0
    args, pre64 = _case(M, N, K, mode)
    out, pre = ops.linear_residual_layernorm(*args, 1e-12, want_pre=True)
    g, msg = _gate(out, _ref64(args, pre64, 1e-12), mode, f"two-kernel form M{M}-N{N}-K{K}-{mode}", 256)
    print(f"\n[fused-ln two-kernel] {msg}")
    assert torch.equal(pre, ops.linear(args[0], args[1], args[2], capi.EPI_F32))
