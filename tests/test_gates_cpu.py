"""CPU: the per-unit floor gates of tests/gpu_util.py (used by test_gpu_ov7b_width.py) reject the errors a wrong kernel makes and
accept a correctly rounded result.  Reduced shapes, numpy float64 references; the "kernel outputs" are that reference with one
realistic defect planted: a stream-K unit that drops one of its 16 key pieces, one unit whose merge weight is off by 2^-6, one
row's log-sum-exp off by 2e-4, one GEMM tile whose contraction stops short, a dK missing one 64-row query tile's contribution
(the backward gate of test_gpu_backward_m64.py), a dW whose last split-K range is dropped or counted twice, LayerNorm rows whose
statistics miss a chunk of 8 elements (the gate of test_gpu_layernorm_forms.py)."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import memory_path as O
from gpu_util import BWD_BLOCK, attention_bwd_ref64, attention_gate, floor_gate, gemm_gate, layernorm_gate, layernorm_ref64, round_to
from gpu_util import DT, F32_SUM_BLOCK, attn_c32, lse2_offsets, mass_gate, prob_mass_eval, rel_l2_t

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


# ------------------------------------------------------------------------------------------------------------------------------
# mass_gate: the fp32 block gate of the kernels that sum softmax probabilities (tests/test_gpu_probability_mass.py)
MS, MH, MHD, MP = 260, 2, 128, 52        # 260 keys: two 128-key blocks + 4 ragged keys, 8 blocks of 32 (+ 4), 5 frames of 52
MQG, MKG = 28, 4                         # map cells: 28 query rows x 4 keys
LN2 = math.log(2.0)


@functools.lru_cache(maxsize=None)
def _mass_case(R, mode):
    """16-bit N(0,1) operands, the fp32 lse2 a stand-alone pass is handed (float64 log-sum-exp rounded to fp32 + a hashed offset
    per row), and the float64 probabilities p [H, R, S] of the kernels' contract exp2(s c - lse2), built in blocks of 2048 rows"""
    g = torch.Generator().manual_seed(9100 + R)
    q = torch.randn((R, MH * MHD), generator=g).to(DT[mode])
    k = torch.randn((MS, MH * MHD), generator=g).to(DT[mode])
    c = attn_c32(np.float32(1.0) / np.sqrt(np.float32(MHD)))
    s = torch.empty((MH, R, MS), dtype=torch.float64)
    for h in range(MH):
        sl = slice(h * MHD, (h + 1) * MHD)
        for r0 in range(0, R, 2048):
            s[h, r0:r0 + 2048] = q[r0:r0 + 2048, sl].double() @ k[:, sl].double().T
    lse = (torch.logsumexp(s * (c * LN2), dim=2) / LN2).float() + lse2_offsets(MH, R)
    p = torch.exp2(s * c - lse.double()[:, :, None])
    return q, k, lse, c, s, p


def _mass_defects(R, lse, c, s, p):
    """column sums [H, S] (float64) of wrong kernels: the reference with one defect each, in head 1"""
    col = p.sum(1)
    last_tile = (R - 1) // 64 * 64                        # first row of the ragged last 64-query tile
    out = {}

    def edit(name, h, keys, delta):
        bad = col.clone()
        bad[h, keys] += delta
        out[name] = bad
    edit("last query row missing from a 32-key block", 1, slice(32, 64), -p[1, R - 1, 32:64])
    edit("a row counted twice in a 32-key block", 1, slice(64, 96), p[1, 64, 64:96])
    edit("a 64-query tile missing from a (128-key block, head) unit", 1, slice(128, 256), -p[1, 64:128, 128:256].sum(0))
    edit("third plane (the last tile's rows) of a three-plane sum dropped", 1, slice(0, 128), -p[1, last_tile:, :128].sum(0))
    r = next(r for r in range(65, R - 1) if abs(float(lse[1, r] - lse[1, r + 1])) >= 0.25)
    edit("a row weighted with the lse2 of the row after it", 1, slice(0, MS),
         torch.exp2(s[1, r] * c - lse[1, r + 1].double()) - p[1, r])
    edit("a padded zero row added with the next head's lse2", 0, slice(128, 256),
         torch.exp2(-lse[1, 0].double()).expand(128))
    return col, out


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("R", [200, 12544])
def test_mass_gate_resolves_one_query_row(R, mode):
    """Column sums per block of 32 keys (one wave of attn_colsum3_kernel), frame scores per frame, map cells per key group.
    Accepted: float64 rounded to fp32, the torch fp32 evaluation, and at R = 200 an fp32 evaluation that adds 64-row tiles in
    order (another summation order).  Rejected at R = 200 and at R = 12 544, where one row is ~1e-4 of a column sum and the
    whole-tensor gate of 1e-3 passes it: every defect of `_mass_defects`, a 4-key group credited to the next frame, a map
    column rotated by one key group."""
    q, k, lse, c, s, p = _mass_case(R, mode)
    col, bad = _mass_defects(R, lse, c, s, p)
    f32 = prob_mass_eval(q, k, lse, MH, MHD, c, torch.float32)
    assert rel_l2_t(prob_mass_eval(q, k, lse, MH, MHD, c), col) < 1e-14
    for name, got in (("float64 rounded to fp32", col.float()), ("torch fp32", f32)):
        g = mass_gate(name, got, col, f32, 32)
        print(g)
        assert g.ok and g.worst <= 1.0 and g.floor < 1e-6, str(g)
    if R == 200:
        g = mass_gate("fp32, 64-row tiles added in order", prob_mass_eval(q, k, lse, MH, MHD, c, torch.float32, rows=64), col, f32, 32)
        print(g)
        assert g.ok, str(g)
    for name, b in bad.items():
        g = mass_gate(name, b.float(), col, f32, 32)
        print(g, f"whole tensor rel-L2 {rel_l2_t(b, col):.1e}")
        assert not g.ok and g.worst > 10 * F32_SUM_BLOCK, str(g)
        if R == 12544 and "row" in name and "tile" not in name:
            assert rel_l2_t(b, col) < 1e-3, name                  # a single row: under the whole-tensor gate
    # a ragged last block of 4 keys is merged into the block before it: 8 blocks of 32, the last one 36 keys
    b = col.clone()
    b[1, -1] *= 1.0001
    g = mass_gate("last key", b.float(), col, f32, 32)
    assert not g.ok and g.where == (1, 7), str(g)

    # frame scores: [F] = sum over heads and the frame's keys / P
    frames = lambda x: x.view(MH, MS // MP, MP).sum(dim=(0, 2)) / MP
    sc, sc32 = frames(col), frames(f32)
    assert mass_gate("scores", sc.float(), sc, sc32, 1).ok
    moved = p[:, :, 2 * MP - 4:2 * MP].sum() / MP                  # the last 4 keys of frame 1, all heads
    b = sc.clone()
    b[1] -= moved
    b[2] += moved
    g = mass_gate("a 4-key group credited to the next frame", b.float(), sc, sc32, 1)
    print(g)
    assert not g.ok and g.where[1] in (1, 2), str(g)
    b = sc.clone()
    b[4] -= p[:, R - 1, 4 * MP:].sum() / MP
    g = mass_gate("last query row missing from the last frame", b.float(), sc, sc32, 1)
    print(g)
    assert not g.ok and g.where == (0, 4), str(g)               # (blocks of one entry: the last one is no ragged tail)

    # maps: [H, query groups, key groups]
    m64 = prob_mass_eval(q, k, lse, MH, MHD, c, torch.float64, MQG, MKG)
    m32 = prob_mass_eval(q, k, lse, MH, MHD, c, torch.float32, MQG, MKG)
    assert tuple(m64.shape) == (MH, -(-R // MQG), MS // MKG) and rel_l2_t(m64.sum(1), col.view(MH, -1, MKG).sum(2)) < 1e-14
    assert mass_gate("map", m64.float(), m64, m32, 1).ok
    b = m64.clone()
    b[1, 3] = torch.roll(b[1, 3], -1)                              # output column j holds key group j + 1
    g = mass_gate("a map row rotated by one key group", b.float(), m64, m32, 1)
    print(g)
    assert not g.ok and g.where[0] == 1 * m64.shape[1] + 3, str(g)
    # one query row per cell: a block is a single exponent and torch's own error is no floor for another correct evaluation;
    # the expected magnitude of the fp32 rounding points is.  The emulation that rounds where the kernels round passes it at 2.7 .. 3.6 x
    # (against torch's floor it reads 8.5 .. 10.4 x), and a rotated row is rejected
    one64 = prob_mass_eval(q, k, lse, MH, MHD, c, torch.float64, 1, MKG)
    one32 = prob_mass_eval(q, k, lse, MH, MHD, c, torch.float32, 1, MKG)
    emu = prob_mass_eval(q, k, lse, MH, MHD, c, torch.float64, 1, MKG, rounding="emulate")
    exp = prob_mass_eval(q, k, lse, MH, MHD, c, torch.float64, 1, MKG, rounding="expected", adds=MKG // 4 + 8)
    g = mass_gate("one-row cells, expected-rounding floor: the emulation", emu, one64, exp, 1)
    print(g, mass_gate("... against the torch floor", emu, one64, one32, 1), sep="\n")
    assert g.ok and g.worst > 1.0 and g.floor < 1e-4, str(g)      # of the size of a correct evaluation's error, not far above
    # (torch's CPU GEMM rounds after every one of the 128 products, not after 8 steps of 16: up to ~10 x this floor, printed)
    print(mass_gate("one-row cells, expected-rounding floor: torch fp32", one32, one64, exp, 1))
    b = one64.clone()
    b[1, 3] = torch.roll(b[1, 3], -1)
    assert not mass_gate("one-row cells, a rotated row", b.float(), one64, exp, 1).ok
