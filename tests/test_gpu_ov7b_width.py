"""-m gpu: the OneVision-7B width (hidden 3584, 8 heads of 448) at the BASELINE's 64 memory tokens, where the head_dim-448
kernels fill the chip: R = 64 x 196 = 12 544 query rows, a 32-frame chunk of S = 6 272 keys, evolution over one memory
(S = 12 544), a row batch of two.  Every operator is compared with torch float64 ON THE GPU computed from the same 16-bit
operands (no emulation oracle: it would re-state the kernels' plans), gated per unit of work against floors computed from the
same data (tests/gpu_util.py: the gates and why), and the whole step against the reference's own outputs
(golden/g7_wide64_fullsize.npz).  Measured ratios are printed (-s)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from oracle import memory_path as O
from conftest import load_golden
from gpu_util import (ATTN_UNIT, ATTN_WHOLE, BWD_BLOCK, DT, attention_bwd_ref64, attention_gate, floor_gate, gemm_gate, rel_l2_t,
                      round_to, to_dev, to_np)

pytestmark = pytest.mark.gpu
D, H, HD, P = 3584, 8, 448, 196
LN2 = math.log(2.0)


def _randn(shape, seed, mode, std=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * std).to(DT[mode])


def _plan(R, S, heads):
    info = (ctypes.c_int32 * 4)()
    capi.check(capi.lib().mavlm_attention_hd_plan_info(R, S, heads, HD, info), "plan info")
    return list(info)


def attention_ref64(q, k, v, heads, scale, rows=2048):
    """softmax(q k^T scale) v per head in float64 (row blocks): ctx [R, heads*HD], lse2 [heads, R] (log2 domain)."""
    R = q.shape[0]
    ctx = torch.empty((R, heads * HD), device=q.device, dtype=torch.float64)
    lse2 = torch.empty((heads, R), device=q.device, dtype=torch.float64)
    for h in range(heads):
        sl = slice(h * HD, (h + 1) * HD)
        kh, vh = k[:, sl].double(), v[:, sl].double()
        for r0 in range(0, R, rows):
            s = (q[r0:r0 + rows, sl].double() @ kh.T) * scale
            lse = torch.logsumexp(s, dim=1)
            ctx[r0:r0 + rows, sl] = torch.exp(s - lse[:, None]) @ vh
            lse2[h, r0:r0 + rows] = lse / LN2
    return ctx, lse2


# ------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("mode,R,S,plan", [("bf16", 12544, 6272, [256, 3, 1, 1]), ("fp16", 12544, 6272, [256, 3, 1, 1]),
                                           ("bf16", 12544, 12544, [256, 3, 1, 1]), ("bf16", 25088, 6272, [256, 6, 1, 1])],
                         ids=["chunk32-bf16", "chunk32-fp16", "evolution-bf16", "rows25088-bf16"])
def test_attention_forward_default_plan_vs_fp64(mode, R, S, plan):
    """attn_fwd_hd2_kernel on the default (untuned) levelled stream-K plan: 784 units (1 568 at 25 088 rows: one video over one K/V
    with the unit count and cuts of a row batch of two, whose (video, head) pairs the plan counts like 16 heads; the per-video
    K/V addressing of a real batch is exercised by the step-level row-batch tests) = whole rounds + the remainder cut into 2^k key pieces merged by
    attn_combine_hd_sk_kernel.  Adversarial rows inside the CUT units: one whose maximum jumps inside the last piece's key range,
    one with all-equal logits, one with logits x 8.  Same bits on a second launch."""
    assert _plan(R, S, H) == plan
    if R == 25088:
        assert _plan(12544, S, 2 * H) == plan                      # the row batch of two: the same unit count, the same cuts
    G, full = plan[0], plan[1]
    units, nqb, nt = (R // 128) * H, R // 128, -(-S // 32)
    rem = units - full * G
    assert G % rem == 0
    pieces = G // rem                                              # one level: `rem` units cut `pieces` ways
    last = units - 1                                               # the last cut unit: (head, query block)
    hc, qb = divmod(last, nqb)
    lo = ((pieces - 1) * nt // pieces) * 32                        # first key of its last piece
    assert full * G <= last and lo > 0
    W = H * HD
    q, k, v = _randn((R, W), 1, mode), _randn((S, W), 2, mode), _randn((S, W), 3, mode)
    sl = slice(hc * HD, (hc + 1) * HD)
    r_jump, r_flat, r_big = qb * 128 + 77, qb * 128 + 5, qb * 128 - 128 + 40   # (the last is in the previous cut unit)
    kj = lo + (S - lo) // 2
    k[kj, sl] = q[r_jump, sl] * 2                                  # powers of two: the operands stay on the 16-bit grid
    q[r_flat] = 0
    q[r_big] *= 8
    scale = ops.attn_scale(HD)
    ctx, lse = ops.attention(q, k, v, H, want_lse=True, head_dim=HD, scale=scale)
    again, lse_again = ops.attention(q, k, v, H, want_lse=True, head_dim=HD, scale=scale)
    assert torch.equal(again, ctx) and torch.equal(lse_again, lse)
    ref, ref_lse2 = attention_ref64(q, k, v, H, scale)
    assert float(ref_lse2[hc, r_jump] * LN2) > 20.0                # the jump row is dominated by its planted key
    # The x8 row's mass sits on one or two keys.  The deferred rescale keeps a stale row maximum until it grows by
    # 2^RESCALE_H_LOG2 (attention_hd.hip), so the dominant key's unnormalised probability is 2^d (0 <= d < 8), not 1, and its
    # rounding to 16 bits - one unit roundoff u at most, relative - scales the whole row coherently; that row's norm dominates
    # its unit's.  So the row is gated on its own, at its floor + u per head, and the units at ATTN_UNIT x floor with that row
    # taken at its rounded exact value; the whole-tensor gate and lse2 include it as it is.
    u = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}[mode]
    rest = ctx.clone()
    rest[r_big] = ref[r_big].to(ctx.dtype)
    g, lerr, ok = attention_gate(rest, lse, ref, ref_lse2, H, mode)
    whole = floor_gate("ctx", ctx, ref, 128, HD, mode, ATTN_UNIT, ATTN_WHOLE).whole
    big = []
    for h in range(H):
        hs = slice(h * HD, (h + 1) * HD)
        e, f = rel_l2_t(ctx[r_big, hs], ref[r_big, hs]), rel_l2_t(round_to(ref[r_big, hs], mode), ref[r_big, hs])
        big.append((e, f))
    rows = {"jump": r_jump, "flat": r_flat, "x8": r_big}
    per_row = {n: rel_l2_t(ctx[r, sl], ref[r, sl]) / max(rel_l2_t(round_to(ref[r, sl], mode), ref[r, sl]), 1e-300)
               for n, r in rows.items()}
    worst_big = max(e / (f + u) for e, f in big)
    print(f"\n[{mode} R={R} S={S}] plan {plan}: {pieces}-way cut units {full * G}..{units - 1}; {g} (x8 row at its rounded "
          f"value); whole tensor as computed {whole:.3f} x floor; worst lse2 error {lerr:.2e}; x8 row: worst head "
          f"{max(e / f for e, f in big):.2f} x floor = {worst_big:.2f} x (floor + u); adversarial rows (err / floor, head {hc}): "
          + ", ".join(f"{n} {x:.2f}" for n, x in per_row.items()))
    assert ok and whole <= ATTN_WHOLE, (str(g), whole, lerr)
    assert worst_big <= 1.0, big


# -------------------------------------------------------------------------------------------------------------------- GEMMs
def _bias(n, seed, mode):
    return _randn((n,), seed, mode, 0.5).float()


@pytest.mark.parametrize("M", [12544, 25088], ids=["video", "rowbatch2"])
def test_gemms_at_m64_shapes_vs_fp64(M):
    """The GEMMs of a formation layer at M = 64 (the persistent kernel with the XCD-blocked tile order, N >= 2048): the q / k / v
    projections (bias), MLP up 12544 x 14336 x 3584 (bias + ReLU), MLP down 12544 x 3584 x 14336 in both fp32 epilogues (plain
    and + residual) - 16-bit outputs per 256 x 256 tile within GEMM_TILE x floor, fp32 outputs within GEMM_F32_TILE rel-L2."""
    mode = "bf16"
    x = _randn((M, D), 11, mode)
    w_up, w_dn, w_q = _randn((4 * D, D), 12, mode, 1 / 64), _randn((D, 4 * D), 13, mode, 1 / 128), _randn((D, D), 14, mode, 1 / 64)
    b_up, b_dn, b_q = _bias(4 * D, 15, mode), _bias(D, 16, mode), _bias(D, 17, mode)
    res = _randn((M, D), 18, mode)
    out = []

    def check(name, got, ref, m):
        worst, ok = gemm_gate(got, ref, m)
        out.append(f"{name} {worst:.3g}")
        assert ok, (name, worst)

    q = ops.linear(x, w_q, b_q, capi.EPI_BIAS)
    check("q-proj (x floor)", q, x.double() @ w_q.double().T + b_q.double(), mode)
    del q
    h = ops.linear(x, w_up, b_up, capi.EPI_RELU)
    check("up+relu (x floor)", h, torch.relu(x.double() @ w_up.double().T + b_up.double()), mode)
    dn64 = h.double() @ w_dn.double().T + b_dn.double()
    check("down fp32 (rel-L2)", ops.linear(h, w_dn, b_dn, capi.EPI_F32), dn64, None)
    check("down+res fp32 (rel-L2)", ops.linear(h, w_dn, b_dn, capi.EPI_RES_F32, residual=res), dn64 + res.double(), None)
    print(f"\n[GEMM M={M}] worst tile: " + "; ".join(out))


def _layernorm64(z, gamma, beta, eps):
    mu = z.mean(dim=1, keepdim=True)
    var = (z - mu).square().mean(dim=1, keepdim=True)
    return (z - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


@pytest.mark.parametrize("fused", [0, 2], ids=["two-kernel", "fused-hook"])
def test_dense_residual_layernorm_k14336_vs_fp64(fused, request):
    """The MLP's Residual block at N = 3584, K = 14336, M = 12544: out = LayerNorm(h W^T + b + res) - the default two-kernel form
    and the fused kernel through its test hook (mavlm_set_fused_layernorm(2): rows up to 4096 columns).  16-bit output per tile
    within GEMM_TILE x floor; the fp32 pre-activation within GEMM_F32_TILE."""
    mode, M, N, K, eps = "bf16", 12544, D, 4 * D, 1e-12
    lib = capi.lib()
    capi.check(lib.mavlm_set_fused_layernorm(fused), "fused layernorm")
    request.addfinalizer(lambda: lib.mavlm_set_fused_layernorm(1))
    assert (lib.mavlm_linear_ln_ws_bytes(M, N, K) > 0) == (fused == 2)
    h = torch.relu(_randn((M, K), 21, mode))
    w, b = _randn((N, K), 22, mode, 1 / 128), _bias(N, 23, mode)
    res = _randn((M, N), 24, mode)
    gamma, beta = (1 + _randn((N,), 25, mode, 0.125)).float(), _bias(N, 26, mode)
    out, pre = ops.linear_residual_layernorm(h, w, b, res, gamma, beta, eps, want_pre=True)
    pre64 = h.double() @ w.double().T + b.double()
    worst_pre, ok_pre = gemm_gate(pre, pre64)
    worst, ok = gemm_gate(out, _layernorm64(pre64 + res.double(), gamma, beta, eps), mode)
    print(f"\n[dense+LN K={K} {'fused' if fused else 'two-kernel'}] worst tile {worst:.3f} x floor; pre fp32 {worst_pre:.2e}")
    assert ok and ok_pre, (worst, worst_pre)


# ----------------------------------------------------------------------------------------------------------------- backward
# the training path's formation at M = 8 over a 32-frame chunk: R = 8 x 196 query rows, S = 32 x 196 keys; and the M = 64 shape
@pytest.mark.parametrize("R,S", [(8 * P, 32 * P), (64 * P, 32 * P)], ids=["m8-chunk32", "m64-chunk32"])
def test_attention_bwd_flash_448_vs_fp64(R, S):
    """attn_bwd_hd_kernel (flash style, head_dim 448): dQ per (64-row block, head), dK and dV per (64-key block, head) within
    BWD_BLOCK x the floor of a float64 reference that rounds where the kernels round; then the dQ-only, dK-only and dV-only
    calls (each output's own kernel mode)."""
    mode, W = "bf16", H * HD
    q, k = _randn((R, W), 31, mode, 0.5), _randn((S, W), 32, mode, 0.5)
    v, do = _randn((S, W), 33, mode), _randn((R, W), 34, mode, 0.5)
    scale = ops.attn_scale(HD)
    o, lse = ops.attention(q, k, v, H, want_lse=True, head_dim=HD, scale=scale)
    full = ops.attention_bwd_hd(q, k, v, o, do, lse, H, HD, scale)
    ex, rd = attention_bwd_ref64(q, k, v, do, H, scale, mode, HD)
    gates = []
    for i, name in enumerate(("dQ", "dK", "dV")):
        g = floor_gate(name, full[i], ex[i], 64, HD, rd[i], BWD_BLOCK)
        gates.append(g)
        need = [j == i for j in range(3)]
        one = ops.attention_bwd_hd(q, k, v, o, do, lse, H, HD, scale, *need)[i]
        g1 = floor_gate(name + "-only", one, ex[i], 64, HD, rd[i], BWD_BLOCK)
        gates.append(g1)
        print(f"  {name}-only bit-identical to the full call: {torch.equal(one, full[i])}")
    print(f"\n[bwd R={R} S={S}]\n  " + "\n  ".join(str(g) for g in gates))
    assert all(g.ok for g in gates), [str(g) for g in gates if not g.ok]


# ------------------------------------------------------------------------------------------------------------ whole step
def _projector(M, wseed):
    from test_gpu_path import make_projector
    cfg = O.PathConfig(hidden=D, heads=H, mem_tokens=M, depth=2)
    w = O.make_weights(cfg, seed=wseed)
    return cfg, make_projector(cfg, w)


def _frame_scores_ref64(proj, seg, cfg):
    """float64 formation from the initial memory (layer 0 in full, rounding to 16 bits where the path stores), then the column
    masses of the last layer's attention summed over heads and averaged per frame (MemoryController.py:135-139)."""
    sd = {k: t.double() for k, t in proj.state_dict().items()}
    r = lambda t: round_to(t, "bf16")
    F = seg.shape[0]
    x = seg.reshape(F * P, D).double()
    m = r(sd["initial_memory"] + sd["memory_pos_embed"]).reshape(cfg.mem_tokens * P, D)
    lin = lambda a, pfx: a @ sd[pfx + ".weight"].T + sd[pfx + ".bias"]
    ln = lambda z, pfx: _layernorm64(z, sd[pfx + ".weight"], sd[pfx + ".bias"], cfg.eps)
    scale = ops.attn_scale(HD)
    for layer in range(cfg.depth):
        a = f"layers.{layer}.memory_segment_fusion_attention"
        q, k = r(lin(m, a + ".q_proj")), r(lin(x, a + ".k_proj"))
        if layer == cfg.depth - 1:
            col = torch.zeros(F * P, device=x.device, dtype=torch.float64)
            for h in range(H):
                sl = slice(h * HD, (h + 1) * HD)
                for r0 in range(0, q.shape[0], 2048):
                    col += torch.softmax((q[r0:r0 + 2048, sl] @ k[:, sl].T) * scale, dim=1).sum(dim=0)
            return col.view(F, P).mean(dim=1)
        v = r(lin(x, a + ".v_proj"))
        ctx, _ = attention_ref64(q, k, v, H, scale)
        att = r(ln(lin(r(ctx), a + ".residual.dense") + m, a + ".residual.layernorm"))
        hid = r(torch.relu(lin(att, f"layers.{layer}.mlp.0")))
        m = r(ln(lin(hid, f"layers.{layer}.residual.dense") + att, f"layers.{layer}.residual.layernorm"))


def test_frame_scores_on_the_stream_k_schedule_vs_fp64():
    """M = 64, a 32-frame chunk: the last formation layer (R = 12544, S = 6272) runs the stream-K plan, and the frame scores ride
    on it (tile entries, FT = 1).  They match float64 column masses of that layer within 2 x the floor of their 16-bit storage,
    sum to H * M = 512, and asking for them (or how) leaves the memory bit-identical to the column-sum mode."""
    assert _plan(64 * P, 32 * P, H)[:3] == [256, 3, 1]
    cfg, proj = _projector(64, 76)
    seg = to_dev(O.bf16_round(O.hash_normal_like((32, P, D), 7600)))
    lib = capi.lib()
    got = {}
    try:
        for mode in (1, 0):
            capi.check(lib.mavlm_set_frame_score_mode(mode), "frame score mode")
            proj.memory_cache = []
            with torch.no_grad():
                cache, scores = proj(seg)
            got[mode] = (cache[-1].clone(), scores[-1].clone())
    finally:
        lib.mavlm_set_frame_score_mode(1)
    assert torch.equal(got[1][0], got[0][0])
    ref = _frame_scores_ref64(proj, seg, cfg)
    assert abs(float(ref.sum()) - H * 64) < 1e-9 * H * 64
    for mode, (_, sc) in got.items():
        err, floor = rel_l2_t(sc, ref), rel_l2_t(round_to(ref, "bf16"), ref)
        print(f"\n[frame scores M=64, {'tile entries' if mode else 'column-sum pass'}] rel-L2 vs fp64 {err:.2e} = "
              f"{err / floor:.2f} x floor ({floor:.2e}); sum {float(sc.float().sum()):.3f}")
        assert err <= 2.0 * floor
        assert abs(float(sc.float().sum()) - H * 64) < 2e-2 * H * 64


@pytest.mark.parametrize("pfx", ["m64_", "m8_"])
def test_golden_g7_wide64_reference(pfx):
    """The whole step at the 7B width against the REFERENCE (golden/g7_wide64_fullsize.npz): m64_ = 64 memory tokens, chunks of 8
    then 32 frames (step 1: evolution over the FIFO, then formation on 6 272 keys - stream-K schedules); m8_ = 8 memory tokens,
    two 32-frame chunks (the split-KV small grid).  The G7 gates (test_gpu_path._g7_gates) per step, single video and a row batch
    of two (`BatchedProjector`)."""
    from test_gpu_path import _g7_gates
    from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
    z, m = load_golden("g7_wide64_fullsize.npz")
    c = m["cases"][pfx]
    _, proj = _projector(c["M"], c["wseed"])
    segs = [to_dev(O.bf16_round(O.hash_normal_like((F, P, D), c["segseed0"] + t))) for t, F in enumerate(c["frames"])]
    errs, ref_errs = [], []
    with torch.no_grad():
        proj.memory_cache = []
        for t, seg in enumerate(segs):
            cache, scores = proj(seg)
            mem = to_np(cache[-1]).reshape(-1)
            e, r = _g7_gates(mem[::m["stride"]], mem, to_np(scores[-1]), z, pfx, t, m, f"7B width {pfx}")
            errs.append(e)
            ref_errs.append(r)
        for t in range(1, len(errs)):
            assert errs[t] / errs[t - 1] <= 1.25 * ref_errs[t] / ref_errs[t - 1] + 0.05, (errs, ref_errs)
        bp = BatchedProjector(proj, 2)
        bp.reset()
        for t, seg in enumerate(segs):
            sc = bp.step([seg, seg.clone()])
            for b in range(2):
                mem = to_np(bp.memory_cache(b)[-1]).reshape(-1)
                _g7_gates(mem[::m["stride"]], mem, to_np(sc[b]), z, pfx, t, m, f"7B width {pfx}, row batch video {b}")
