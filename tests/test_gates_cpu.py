"""CPU: the per-unit floor gates of tests/gpu_util.py (used by test_gpu_ov7b_width.py) reject the errors a wrong kernel makes and
accept a correctly rounded result.  Reduced shapes, numpy float64 references; the "kernel outputs" are that reference with one
realistic defect planted: a stream-K unit that drops one of its 16 key pieces, one unit whose merge weight is off by 2^-6, one
row's log-sum-exp off by 2e-4, one GEMM tile whose contraction stops short, a dK missing one 64-row query tile's contribution
(the backward gate of test_gpu_backward_m64.py), a dW whose last split-K range is dropped or counted twice, LayerNorm rows whose
statistics miss a chunk of 8 elements (the gate of test_gpu_layernorm_forms.py)."""
import math

import numpy as np
import pytest
import torch

from oracle import memory_path as O
from gpu_util import BWD_BLOCK, attention_bwd_ref64, attention_gate, floor_gate, gemm_gate, layernorm_gate, layernorm_ref64, round_to

R, S, H, HD = 8192, 512, 2, 64         # 64 128-query units per head; a unit's keys in 16 pieces of 32
PIECES = 16


def _inputs():
    q = O.bf16_round(O.hash_normal_like((R, H * HD), 11)).astype(np.float64)
    k = O.bf16_round(O.hash_normal_like((S, H * HD), 12)).astype(np.float64)
    v = O.bf16_round(O.hash_normal_like((S, H * HD), 13)).astype(np.float64)
    return q, k, v


def _attention64(q, k, v, keys=slice(None)):
    """ctx [rows, H*HD], lse2 [H, rows] (log2 domain) in float64 over the key subset `keys`."""
    ctx = np.empty((q.shape[0], H * HD))
    lse2 = np.empty((H, q.shape[0]))
    for h in range(H):
        sl = slice(h * HD, (h + 1) * HD)
        s = q[:, sl] @ k[keys, sl].T / math.sqrt(HD)
        m = s.max(axis=1, keepdims=True)
        p = np.exp(s - m)
        l = p.sum(axis=1, keepdims=True)
        ctx[:, sl] = (p @ v[keys, sl]) / l
        lse2[h] = (m[:, 0] + np.log(l[:, 0])) / math.log(2.0)
    return ctx, lse2


def _ok(ctx, lse2, ref, ref_lse2, whole=None):
    g, lerr, ok = attention_gate(ctx, lse2, ref, ref_lse2, H, "bf16")
    print(g, f"lse2 {lerr:.1e}")
    if whole is not None:
        whole.append(g.whole)
    return ok


def test_attention_gate_accepts_the_rounded_reference():
    ref, lse2 = _attention64(*_inputs())
    assert _ok(O.bf16_round(ref.astype(np.float32)), lse2.astype(np.float32), ref, lse2)


def test_attention_gate_rejects_a_unit_missing_one_key_piece():
    q, k, v = _inputs()
    ref, lse2 = _attention64(q, k, v)
    keep = np.ones(S, bool)
    keep[5 * S // PIECES:6 * S // PIECES] = False             # unit (rows 128..255, head 1) loses piece 5 of 16
    c, l = _attention64(q[128:256], k, v, keep)
    bad, bad_lse = ref.copy(), lse2.copy()
    bad[128:256, HD:] = c[:, HD:]
    bad_lse[1, 128:256] = l[1]
    assert not _ok(O.bf16_round(bad.astype(np.float32)), bad_lse.astype(np.float32), ref, lse2)
    assert not _ok(O.bf16_round(bad.astype(np.float32)), lse2.astype(np.float32), ref, lse2)    # the context alone


def test_attention_gate_rejects_a_misweighted_unit():
    ref, lse2 = _attention64(*_inputs())
    bad = ref.copy()
    bad[:128, HD:] *= 1.0 + 2.0 ** -6
    whole = []
    assert not _ok(O.bf16_round(bad.astype(np.float32)), lse2.astype(np.float32), ref, lse2, whole)
    assert whole[0] < 1.5              # one unit in 128: the whole-tensor gate alone would let it through


def test_attention_gate_rejects_one_row_of_lse2():
    ref, lse2 = _attention64(*_inputs())
    bad = lse2.copy()
    bad[0, 77] += 2e-4
    assert not _ok(O.bf16_round(ref.astype(np.float32)), bad.astype(np.float32), ref, lse2)


def test_gemm_tile_gate():
    M, N, K = 512, 768, 1024
    a = O.bf16_round(O.hash_normal_like((M, K), 21)).astype(np.float64)
    w = O.bf16_round(O.hash_normal_like((N, K), 22)).astype(np.float64)
    ref = a @ w.T
    bad = ref.copy()
    bad[256:512, 256:512] = a[256:512, :K - 32] @ w[256:512, :K - 32].T      # one tile's K range stops 32 short
    assert gemm_gate(O.bf16_round(ref.astype(np.float32)), ref, "bf16")[1]
    assert not gemm_gate(O.bf16_round(bad.astype(np.float32)), ref, "bf16")[1]
    assert gemm_gate(ref.astype(np.float32), ref)[1]                                 # fp32 epilogue
    assert not gemm_gate(bad.astype(np.float32), ref)[1]


def test_backward_gate_rejects_a_dk_missing_one_query_tile():
    """dK = scale * dS^T Q sums over every query row: a kernel that skips one 64-row query tile (e.g. a dropped workgroup
    of the row loop) leaves every key block short of 1/64 of its terms.  The per-(64-key block, head) gate against the
    rounded float64 reference rejects it and accepts that reference."""
    rows, keys, tile = 4096, 256, 64
    t = lambda a: torch.from_numpy(O.bf16_round(a).astype(np.float64))
    q, k = t(O.hash_normal_like((rows, H * HD), 31)), t(O.hash_normal_like((keys, H * HD), 32))
    v, do = t(O.hash_normal_like((keys, H * HD), 33)), t(O.hash_normal_like((rows, H * HD), 34, 0.5))
    scale = 1.0 / math.sqrt(HD)
    ex, rd = attention_bwd_ref64(q, k, v, do, H, scale, "bf16", HD, rows=1024)
    keep = torch.ones(rows, dtype=torch.bool)
    keep[7 * tile:8 * tile] = False                          # query tile 7 of 64 contributes nothing
    _, rd_bad = attention_bwd_ref64(q[keep], k, v, do[keep], H, scale, "bf16", HD, rows=1024)
    ok = floor_gate("dK", rd[1], ex[1], 64, HD, rd[1], BWD_BLOCK)
    bad = floor_gate("dK", rd_bad[1], ex[1], 64, HD, rd[1], BWD_BLOCK)
    print(ok, bad, sep="\n")
    assert ok.ok and not bad.ok


def test_tile_gate_rejects_a_dw_with_its_last_split_wrong():
    """dW = dY^T X over K = 6 272 rows in 8 split-K planes of 832 (the last one 448, as mavlm_launch_gemm_splitk cuts it):
    a reduction that drops the last plane or adds it twice is rejected by the per-tile gate; the rounded float64 result
    passes."""
    m, n, k, ksplit = 512, 512, 6272, 832
    a = O.bf16_round(O.hash_normal_like((m, k), 41)).astype(np.float64)
    b = O.bf16_round(O.hash_normal_like((n, k), 42)).astype(np.float64)
    ref = a @ b.T
    lo = (k // ksplit) * ksplit
    assert k - lo == 448
    last = a[:, lo:] @ b[:, lo:].T
    assert gemm_gate(O.bf16_round(ref.astype(np.float32)), ref, "bf16")[1]
    for bad in (ref - last, ref + last):
        assert not gemm_gate(O.bf16_round(bad.astype(np.float32)), ref, "bf16")[1]
        one = ref.copy()
        one[256:, :256] = bad[256:, :256]                   # in one 256 x 256 tile only
        assert not gemm_gate(O.bf16_round(one.astype(np.float32)), ref, "bf16")[1]


def _layernorm_defects(x, res, g, b, eps):
    """float64 outputs of three wrong kernels on rows z = x + res: the mean taken over D - 8 elements (a dropped chunk), the
    last 8 residual elements not added, the variance divided by D + 8; and `dropped sum`: the chunk missing from the sum only
    (mean = sum over D - 8 elements / D), what dropping a chunk from the kernels' first pass gives."""
    d = x.shape[1]
    z = x.astype(np.float64) + res
    ln = lambda zz, mean, var: torch.from_numpy((zz - mean) / np.sqrt(var + eps) * g + b)
    mu, var = z.mean(1, keepdims=True), z.var(1, keepdims=True)
    nr = z.copy()
    nr[:, -8:] = x[:, -8:]
    return {"mean over D - 8": ln(z, z[:, :-8].mean(1, keepdims=True), var),
            "last 8 residual elements missing": ln(nr, nr.mean(1, keepdims=True), nr.var(1, keepdims=True)),
            "variance / (D + 8)": ln(z, mu, var * d / (d + 8)),
            "dropped sum": ln(z, z[:, :-8].sum(1, keepdims=True) / d, var)}


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_layernorm_gate_rejects_rows_with_wrong_statistics(mode):
    """The gate of tests/test_gpu_layernorm_forms.py (per block of 4 rows, BWD_BLOCK x the floor of float64 rounded once to the
    output grid) on the rows of that test: x = 3 N(0,1) + 0.5 and x = 64 + N(0,1), a 16-bit residual.  The rounded float64
    result passes at a ratio of exactly 1; the outputs of `_layernorm_defects` are rejected
      - with ONE row of 37 wrong (a quarter of its block) at D = 256 on the first kind of rows, and
      - with every row wrong, as a kernel defect is, at D = 512 and 1024 on both kinds.
    A defect in 8 of D elements of the statistics moves the output by ~8 / D, the floor is 2^-9 / 2^-12 whatever D: at D = 4096
    the bf16 gate no longer sees a mean over D - 8 elements or a variance over D + 8 (1.1 - 1.2 x floor with every row wrong),
    the fp16 gate does (4.3 x or more) - one reason the GPU test runs both types - and both see the missing residual elements
    and, on the rows of 64 + N(0,1), the chunk dropped from the sum (the shift of the mean is 8 x 64 / D): asserted at 4096."""
    rows, eps, bad_row = 37, 1e-12, 21
    for d in (256, 512, 1024, 4096):
        g = 1.0 + O.hash_uniform((d,), 52, -0.1, 0.1).astype(np.float64)
        b = O.hash_uniform((d,), 53, -0.1, 0.1).astype(np.float64)
        res = round_to(O.hash_normal_like((rows, d), 54), mode).numpy()
        for kind, x in (("3 N + 0.5", O.hash_normal_like((rows, d), 51) * 3.0 + 0.5), ("64 + N", O.hash_normal_like((rows, d), 55) + 64.0)):
            x = x.astype(np.float32)
            ref = layernorm_ref64(x, res, g, b, eps)
            good = layernorm_gate("rounded float64", round_to(ref, mode), ref, mode)
            assert good.ok and good.worst == 1.0, str(good)
            for name, out in _layernorm_defects(x, res, g, b, eps).items():
                every = layernorm_gate(f"D {d} {kind}: {name}, every row", round_to(out, mode), ref, mode)
                one = ref.clone()
                one[bad_row] = out[bad_row]
                single = layernorm_gate(f"D {d} {kind}: {name}, one row", round_to(one, mode), ref, mode)
                print(every, single, sep="\n")
                if d == 256 and kind == "3 N + 0.5":
                    assert not single.ok and single.where == (bad_row // 4, 0), str(single)
                if d in (512, 1024):
                    assert not every.ok, str(every)
                if d == 4096 and (mode == "fp16" or name == "last 8 residual elements missing" or
                                  (name == "dropped sum" and kind == "64 + N")):
                    assert not every.ok, str(every)
