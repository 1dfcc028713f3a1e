"""CPU: the per-unit floor gates of tests/gpu_util.py (used by test_gpu_ov7b_width.py) reject the errors a wrong kernel makes and
accept a correctly rounded result.  Reduced shapes, numpy float64 references; the "kernel outputs" are that reference with one
realistic defect planted: a stream-K unit that drops one of its 16 key pieces, one unit whose merge weight is off by 2^-6, one
row's log-sum-exp off by 2e-4, one GEMM tile whose contraction stops short, a dK missing one 64-row query tile's contribution
(the backward gate of test_gpu_backward_m64.py), a dW whose last split-K range is dropped or counted twice, LayerNorm rows whose
statistics miss a chunk of 8 elements (the gate of test_gpu_layernorm_forms.py), and the defects a row of the fused dense + residual +
LayerNorm epilogue can have on its own (the gate of test_gpu_fused_layernorm.py; a restatement of that epilogue in fp32)."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import memory_path as O
from gpu_util import BWD_BLOCK, attention_bwd_ref64, attention_gate, floor_gate, gemm_gate, layernorm_gate, layernorm_ref64, round_to
from gpu_util import DT, F32_SUM_BLOCK, attn_c32, lse2_offsets, mass_gate, prob_mass_eval, rel_l2_t
from gpu_util import block_rel_l2, fused_ln_gate, fused_ln_inputs, fused_ln_pattern, fused_ln_ref64

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


# ------------------------------------------------------------------------------------------------------------------------------
# fused_ln_gate: the fused dense + residual + LayerNorm epilogue (EPI_LN of csrc/gemm256.hip), restated from its description - per
# 256-column tile the mean and the centred sum of squares of a row, Chan's merge of the tiles in tile order, the normalisation -
# in fp32 (what the kernel computes) or float64, with one defect in ONE row where asked
FL_M, FL_K = 96, 64
FL_ROW = 37                      # the row the single-row defects sit in: block 9 of the 4-row blocks


def _fl_partner(M, N, row):
    """the tile whose pair the single-row defects replace: the first tile of `row` whose planted offset is not zero (read as zeros,
    such a tile's mean goes missing) and differs from that of row + 16 - any tile in a real launch; the pattern leaves one in
    every row but those whose offsets all equal the other row's"""
    _, o = fused_ln_pattern(M, N // 256)
    return next(t for t in range(N // 256) if o[row, t] != 8 and o[row, t] != o[row + 16, t])


def _fused_epilogue(z, gamma, beta, eps, dt, defect=None, row=FL_ROW, tile=1):
    """z = dense + bias + residual [M, N] -> LayerNorm(z) gamma + beta [M, N], all arithmetic in `dt`"""
    z, gamma, beta = z.to(dt), gamma.to(dt), beta.to(dt)
    M, N = z.shape
    ntn = N // 256
    zt = z.view(M, ntn, 256)
    mk = zt.sum(dim=2) / 256.0                                          # [M, ntn] per-tile mean
    qk = (zt - mk[:, :, None]).square().sum(dim=2)                      # per-tile centred sum of squares
    if defect == "partner pair from row + 16":
        mk, qk = mk.clone(), qk.clone()
        mk[row, tile], qk[row, tile] = mk[row + 16, tile], qk[row + 16, tile]
    if defect == "partner pair read as zeros":
        mk, qk = mk.clone(), qk.clone()
        mk[row, tile] = qk[row, tile] = 0.0
    msum = torch.zeros(M, dtype=dt)
    for k in range(ntn):
        msum = msum + mk[:, k]
    mean = msum / float(ntn)
    if defect == "mean over ntn - 1 tiles":
        mean = mean.clone()
        mean[row] = sum(mk[row, k] for k in range(ntn - 1)) / float(ntn - 1)
    m2 = torch.zeros(M, dtype=dt)
    for k in range(ntn):
        d = mk[:, k] - mean
        between = 256.0 * d * d
        if defect == "between-tile term dropped":
            between[row] = 0.0
        m2 = m2 + (qk[:, k] + between)
    rstd = 1.0 / torch.sqrt(m2 / float(N) + eps)
    if defect == "last row with the statistics of the row before":
        mean, rstd = mean.clone(), rstd.clone()
        mean[M - 1], rstd[M - 1] = mean[M - 2], rstd[M - 2]
    out = (z - mean[:, None]) * rstd[:, None] * gamma + beta
    if defect == "slab with the gamma of the next 16 columns":
        r0, c0 = 16 * (row // 16), 256 * tile + 64
        out[r0:r0 + 16, c0:c0 + 64] = (z[r0:r0 + 16, c0:c0 + 64] - mean[r0:r0 + 16, None]) * rstd[r0:r0 + 16, None] \
            * gamma[c0 + 16:c0 + 80] + beta[c0:c0 + 64]
    return out


FL_DEFECTS = ("between-tile term dropped", "partner pair from row + 16", "partner pair read as zeros", "mean over ntn - 1 tiles",
              "last row with the statistics of the row before", "slab with the gamma of the next 16 columns")


@functools.lru_cache(maxsize=None)
def _fl_case(N, mode, planted):
    x, w, b, res, gamma, beta = fused_ln_inputs(FL_M, N, FL_K, mode, 4000 + N, planted=planted, device="cpu")
    z32 = x.float() @ w.float().T + b + res.float()                      # the fp32 accumulator + bias + residual
    return z32, gamma, beta, fused_ln_ref64(x, w, b, res, gamma, beta, 1e-12)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("N", [512, 1024, 4096])
def test_fused_ln_gate_on_the_restated_epilogue(N, mode):
    """96 rows, K = 64, planted residual.  Accepted at 1.0 x floor: the float64 reference rounded to the output grid, and the
    fp32 restatement of the epilogue rounded once.  Rejected, each in ONE row (or one 16 x 64 slab) and at the block that holds it:
    every defect of FL_DEFECTS."""
    z32, gamma, beta, ref = _fl_case(N, mode, True)
    tile = _fl_partner(FL_M, N, FL_ROW)
    g = fused_ln_gate(round_to(ref, mode), ref, mode)
    assert g.ok and g.worst == 1.0 and g.whole == 1.0, str(g)
    assert rel_l2_t(_fused_epilogue(z32, gamma, beta, 1e-12, torch.float64), ref) < 1e-6      # (the operands' fp32 product only)
    g = fused_ln_gate(_fused_epilogue(z32, gamma, beta, 1e-12, torch.float32).to(DT[mode]), ref, mode)
    print(g)
    assert g.ok and g.worst < 1.02 and g.whole < 1.01, str(g)
    for name in FL_DEFECTS:
        bad = _fused_epilogue(z32, gamma, beta, 1e-12, torch.float32, name, FL_ROW, tile).to(DT[mode])
        g = fused_ln_gate(bad, ref, mode)
        print(f"N {N} {mode} {name}: {g}")
        assert not g.ok and g.worst > 3 * BWD_BLOCK, str(g)          # (the mildest: a tile of offset sigma / 2 read as zeros among 16, 6.5 x)
        if "last row" in name:
            assert g.where[0] == (FL_M - 1) // 4, str(g)
        elif "slab" in name:
            assert g.where[0] // 4 == FL_ROW // 16 and g.where[1] == tile, str(g)
        else:
            assert g.where[0] == FL_ROW // 4, str(g)


def test_fused_ln_gate_needs_the_planted_rows():
    """Why the inputs are planted.  One row in every block of 4 drops the between-tile term of the merge (the blocks are gated
    independently: 24 single-row defects at once).  On plain N(0,1) operands the tile means of a row differ by sigma / 16 and nearly
    every block passes the bf16 gate (measured: all of 24 at N = 512 and 4096, 23 at N = 1024, worst 1.60 x floor) - with a quarter
    of all rows wrong the whole tensor reads 1.14 x floor at most, under the limit as well; on the planted rows every block is rejected, the mildest at 6.5 x floor."""
    rows = torch.arange(1, FL_M, 4)
    for N in (512, 1024, 4096):
        ratios = {}
        for planted in (False, True):
            z32, gamma, beta, ref = _fl_case(N, "bf16", planted)
            bad = _fused_epilogue(z32, gamma, beta, 1e-12, torch.float32, FL_DEFECTS[0], rows).to(torch.bfloat16)
            ratio = (block_rel_l2(bad, ref, 4, 256) / block_rel_l2(round_to(ref, "bf16"), ref, 4, 256)).max(dim=1).values
            g = fused_ln_gate(bad, ref, "bf16")
            assert float(ratio.max()) == g.worst
            print(f"N {N} planted {planted}: per block {float(ratio.min()):.2f} .. {float(ratio.max()):.2f} x floor, "
                  f"{int((ratio <= BWD_BLOCK).sum())} of {ratio.numel()} pass; {g}")
            ratios[planted] = (ratio, g)
        assert float((ratios[False][0] <= BWD_BLOCK).float().mean()) >= 0.9 and ratios[False][1].whole < BWD_BLOCK, str(ratios[False][1])
        assert float(ratios[True][0].min()) > 4 * BWD_BLOCK, str(ratios[True][1])
