"""-m gpu: the training backward at the headline width (hidden 1024, 8 heads of 128) with 64 memory tokens and 32-frame chunks:
R = 64 x 196 = 12 544 query rows, a chunk of S = 6 272 keys, evolution over one memory (S = 12 544), a 5-frame trailing chunk
(S = 980, not a multiple of 64).

Every operator of the backward is compared with torch float64 ON THE GPU computed from the same 16-bit operands, gated per unit
of work against floors computed from the same data (tests/gpu_util.py: the gates and why); the shapes are those a training step
at M = 64 issues, and a live step checks that they are all covered.  The whole step is compared with oracle/torch_path.py in
float64 on the GPU, inside the envelope of the same restatement under torch bf16 autograd (the reference's own arithmetic),
and that GPU-built envelope is tied to the one the reference stored (golden/g8_grads_d1024.npz).  Measured ratios are printed
(-s)."""
import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from oracle import memory_path as O
from oracle import torch_path as TP
from conftest import load_golden
from gpu_util import (BWD_BLOCK, DT, attention_bwd_ref64, f32_sum_gate, floor_gate, gemm_gate)
from test_gpu_backward_path import _cotangents, _hip_grads, _segs
from test_gpu_path import make_projector

pytestmark = pytest.mark.gpu
D, H, HD, P, M = 1024, 8, 128, 196, 64
R = M * P                                      # 12 544 memory rows
CHUNKINGS = ([32, 32], [32, 5])                # formation, evolution + formation; the second with a 5-frame trailing chunk


def _randn(shape, seed, mode, std=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * std).to(DT[mode])


# ------------------------------------------------------------------------- the shapes a training step at M = 64 issues
# (dtype, rows R, keys S, heads): ops.attention_bwd
ATTN_CASES = {"formation": ("bf16", R, 32 * P), "evolution": ("bf16", R, R), "tail5": ("bf16", R, 5 * P),
              "formation-fp16": ("fp16", R, 32 * P), "adversarial": ("bf16", R, 32 * P)}
# (M, N, K) of ops.matmul_nt_splitk(a [M, K], b [N, K]) = dW^T-shaped products dY^T X (K = rows padded to 64)
SPLITK_SHAPES = [(4096, 1024, 32 * P), (4096, 1024, 1024), (1024, 1024, R), (4096, 1024, R), (1024, 4096, R), (2048, 1024, R)]
# (M, N, K) of ops.matmul_nt(dy [M, K], W^T [N, K]) = the dX products
MATMUL_NT_SHAPES = [(R, 1024, 1024), (R, 1024, 4096), (R, 4096, 1024), (R, 1024, 2048)]
# (rows, D, residual) of ops.layernorm_bwd
LN_SHAPES = [(R, D, True), (R, D, False), (5 * P, D, True), (5 * P, D, False)]
NEEDS = [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]

RECORDED = ("attention_bwd", "matmul_nt_splitk", "matmul_nt", "layernorm_bwd")


def _key(name, a, kw):
    """The shape of one call as the tests above parametrise it."""
    if name == "attention_bwd":
        q, k, heads = a[0], a[1], a[6]
        pos = a[7:10]
        need = tuple(bool(pos[i]) if i < len(pos) else bool(kw.get(n, True))
                     for i, n in enumerate(("need_dq", "need_dk", "need_dv")))
        scale = kw.get("scale")
        assert scale is None or scale == ops.attn_scale(HD)
        return (str(q.dtype), q.shape[0], k.shape[0], heads, need)
    if name == "layernorm_bwd":
        return (str(a[0].dtype), a[1].shape[0], a[1].shape[1], a[2] is not None)
    if name == "matmul_nt_splitk":
        splits = a[2] if len(a) > 2 else kw.get("splits")
        return (str(a[0].dtype), a[0].shape[0], a[1].shape[0], a[0].shape[1], splits)
    return (str(a[0].dtype), a[0].shape[0], a[1].shape[0], a[0].shape[1])


def _tested_keys():
    t = str(torch.bfloat16)
    return {"attention_bwd": {(str(DT[m]), r, s, H, n) for m, r, s in ATTN_CASES.values() for n in NEEDS},
            "matmul_nt_splitk": {(t, m, n, k, None) for m, n, k in SPLITK_SHAPES},
            "matmul_nt": {(t, m, n, k) for m, n, k in MATMUL_NT_SHAPES},
            "layernorm_bwd": {(t, rows, d, res) for rows, d, res in LN_SHAPES}}


def _recording(fn):
    """Run fn() with the backward operators of _ops wrapped to record the shape of every outermost call."""
    shapes = {n: set() for n in RECORDED}
    orig = {n: getattr(ops, n) for n in RECORDED}
    depth = [0]

    def wrap(name):
        f = orig[name]

        def g(*a, **kw):
            if depth[0] == 0:
                shapes[name].add(_key(name, a, kw))
            depth[0] += 1
            try:
                return f(*a, **kw)
            finally:
                depth[0] -= 1
        return g
    for n in RECORDED:
        setattr(ops, n, wrap(n))
    try:
        out = fn()
    finally:
        for n in RECORDED:
            setattr(ops, n, orig[n])
    return out, shapes


_CFG = O.PathConfig(hidden=D, heads=H, mem_tokens=M, depth=2)
_STEPS = {}


def _m64_step(frames):
    """Weights, inputs and the HIP training step (loss, gradients, recorded operator shapes) at M = 64, once per chunking."""
    key = tuple(frames)
    if key not in _STEPS:
        w = O.make_weights(_CFG, seed=64)
        segs = _segs(_CFG, frames, 6400)
        cots = _cotangents(_CFG, len(frames), 6450, 0.05)
        rm = make_projector(_CFG, w, "bf16").train()
        (loss, g, _), shapes = _recording(lambda: _hip_grads(rm, segs, cots, "bf16"))
        del rm
        torch.cuda.empty_cache()
        _STEPS[key] = (w, segs, cots, loss, g, shapes)
    return _STEPS[key]


def test_tested_shapes_cover_the_m64_training_step():
    """One training step at M = 64 per chunking, with ops.attention_bwd / matmul_nt_splitk / matmul_nt / layernorm_bwd
    wrapped: every shape the step issues is one the operator tests of this file gate."""
    tested = _tested_keys()
    for frames in CHUNKINGS:
        shapes = _m64_step(frames)[5]
        print(f"\n[M=64 chunks {frames}] operator shapes issued by the training step:")
        for n in RECORDED:
            print(f"  {n}: {sorted(shapes[n], key=str)}")
            assert shapes[n], n
            missing = shapes[n] - tested[n]
            assert not missing, (n, sorted(missing, key=str))


# ---------------------------------------------------------------------------------------------------- attention backward
_ATTN = {}


def _attn_case(name):
    """Operands, forward (O, lse2) and float64 references (exact, rounded) of one case, built once."""
    if name not in _ATTN:
        mode, r, s = ATTN_CASES[name]
        seed = 100 + 10 * list(ATTN_CASES).index(name)
        W = H * HD
        q, k = _randn((r, W), seed, mode), _randn((s, W), seed + 1, mode)
        v, do = _randn((s, W), seed + 2, mode), _randn((r, W), seed + 3, mode, 0.5)
        info = ""
        if name == "adversarial":
            # one 64-key block whose probabilities underflow fp32 for every row (its logits sit ~180 below every row's
            # maximum: P = exp2(S*c - lse2) = 0 there, and the exact values round to zero on the 16-bit grid) ...
            j0 = 37 * 64
            for h in range(H):
                q[:, h * HD] = 8
                k[j0:j0 + 64, h * HD] = -256
            # ... and rows whose softmax is nearly one-hot (logits x 32, powers of two: the operands stay on the grid): P of
            # their top key is ~1 and dS = P o (dP - delta) cancels almost completely
            onehot = [0, 63, 64 * 97 + 5, 6000, r - 1]
            q[onehot] *= 32
            info = f"underflowing key block {j0 // 64}, one-hot rows {onehot}"
        o, lse = ops.attention(q, k, v, H, want_lse=True)
        scale = ops.attn_scale(HD)
        ex, rd = attention_bwd_ref64(q, k, v, do, H, scale, mode, HD, o=o)
        rd_exact_o = None
        if name == "adversarial":
            rd_exact_o = attention_bwd_ref64(q, k, v, do, H, scale, mode, HD)[1]
            pmax = torch.cat([torch.softmax((q[onehot, h * HD:(h + 1) * HD].double() @ k[:, h * HD:(h + 1) * HD].double().T)
                                            * scale, dim=1).max(dim=1).values for h in range(H)])
            assert float(pmax.median()) > 0.99, pmax                          # the rows are nearly one-hot
            assert not rd[1][j0:j0 + 64].any() and not rd[2][j0:j0 + 64].any()
            assert ex[2][j0:j0 + 64].abs().max() < 1e-60                       # (nonzero in float64, far below the grid)
            info += f"; their top probability per head: median {float(pmax.median()):.6f}, min {float(pmax.min()):.4f}"
        _ATTN[name] = (mode, q, k, v, do, o, lse, ex, rd, rd_exact_o, info)
    return _ATTN[name]


@pytest.mark.parametrize("fused", [0, 1], ids=["dk-dv-separate", "dk-dv-fused"])
@pytest.mark.parametrize("case", list(ATTN_CASES))
def test_attention_bwd_m64_vs_fp64(case, fused, request):
    """attention_bwd.hip (head_dim 128) on the production grids: 98 query tiles by 49 / 98 / 8 key tiles per head.  dQ per
    (64-row block, head), dK and dV per (64-key block, head) within BWD_BLOCK x the floor of a float64 reference that rounds
    where the kernels round (delta from the stored forward output O they read); then the dQ-only, dK-only and dV-only calls
    through the same gate.  Both values of the fused dK + dV switch."""
    lib = capi.lib()
    capi.check(lib.mavlm_set_attention_bwd_fused(fused), "set fused")
    request.addfinalizer(lambda: lib.mavlm_set_attention_bwd_fused(0))
    mode, q, k, v, do, o, lse, ex, rd, rd_exact_o, info = _attn_case(case)
    full = ops.attention_bwd(q, k, v, o, do, lse, H)
    gates, same = [], []
    for i, name in enumerate(("dQ", "dK", "dV")):
        gates.append(floor_gate(name, full[i], ex[i], 64, HD, rd[i], BWD_BLOCK))
        if rd_exact_o is not None:
            g = floor_gate(name, full[i], ex[i], 64, HD, rd_exact_o[i], BWD_BLOCK)
            info += f"\n  (with delta from the exact O rounded to bf16 instead of the stored O, the floor misses the forward's " \
                    f"rounding of the one-hot rows: {name} worst block {g.worst:.3f} x that floor at {g.where})"
        need = [j == i for j in range(3)]
        one = ops.attention_bwd(q, k, v, o, do, lse, H, *need)
        assert all(one[j] is None for j in range(3) if j != i)
        gates.append(floor_gate(name + "-only", one[i], ex[i], 64, HD, rd[i], BWD_BLOCK))
        same.append(f"{name} {torch.equal(one[i], full[i])}")
    print(f"\n[attention bwd {case} {mode} R={q.shape[0]} S={k.shape[0]} fused={fused}] {info}\n  "
          + "\n  ".join(str(g) for g in gates) + "\n  single-output calls bit-identical to the full call: " + ", ".join(same))
    assert all(g.ok for g in gates), [str(g) for g in gates if not g.ok]


# ------------------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("rows,d,with_res", LN_SHAPES, ids=[f"rows{r}-{'res' if x else 'nores'}" for r, _, x in LN_SHAPES])
def test_layernorm_bwd_m64_vs_fp64(rows, d, with_res):
    """layernorm_bwd_kernel: 512 workgroups, each reducing ~25 of the 12 544 rows into its dgamma / dbeta partial, then the
    column sum of the partials.  dz per 64-row block within BWD_BLOCK x the floor of float64 dz rounded to bf16; dgamma and
    dbeta (fp32 sums over all rows) per 256-column block within F32_SUM_BLOCK x the fp32 floor (a plain torch fp32 evaluation
    of the same sums, or the float64 result rounded to fp32 once, whichever is larger)."""
    mode, eps = "bf16", 1e-12
    x = torch.randn((rows, d), generator=torch.Generator(device="cuda").manual_seed(rows + 7), device="cuda") * 1.5 + 0.25
    res = _randn((rows, d), rows + 8, mode) if with_res else None
    dy = _randn((rows, d), rows + 9, mode, 0.7)
    gamma = (1.0 + 0.2 * _randn((d,), rows + 10, mode)).float()
    dz, dg, db = ops.layernorm_bwd(dy, x, res, gamma, eps)
    z = x.double() + (res.double() if with_res else 0.0)
    mu = z.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt((z - mu).square().mean(dim=1, keepdim=True) + eps)
    xh = (z - mu) * rstd
    g = dy.double() * gamma.double()
    dz64 = rstd * (g - g.mean(dim=1, keepdim=True) - xh * (g * xh).mean(dim=1, keepdim=True))
    # plain torch fp32 of the same sums (the fp32 floor)
    z32 = x + (res.float() if with_res else 0.0)
    mu32 = z32.mean(dim=1, keepdim=True)
    xh32 = (z32 - mu32) * torch.rsqrt((z32 - mu32).square().mean(dim=1, keepdim=True) + eps)
    gates = [floor_gate("dz", dz, dz64, 64, d, mode, BWD_BLOCK),
             f32_sum_gate("dgamma", dg, (dy.double() * xh).sum(dim=0), (dy.float() * xh32).sum(dim=0), 256),
             f32_sum_gate("dbeta", db, dy.double().sum(dim=0), dy.float().sum(dim=0), 256)]
    print(f"\n[layernorm bwd rows={rows} D={d} residual={with_res}]\n  " + "\n  ".join(str(g) for g in gates))
    assert all(g.ok for g in gates), [str(g) for g in gates if not g.ok]


# -------------------------------------------------------------------------------------------------- weight-gradient path
@pytest.mark.parametrize("rows,cols", [(R, 1024), (R, 2048), (R, 4096), (32 * P, 4096), (32 * P, 1024), (5 * P, 4096),
                                       (5 * P, 1024)])
def test_transpose_and_rowsum_m64(rows, cols):
    """transpose_kernel at the step's row counts: bit-exact, the pad to 64 rows zero (980 -> 1024); rowsum_kernel (the bias
    gradients, row sums of dY^T) per 256-entry block within F32_SUM_BLOCK x the fp32 floor."""
    x = _randn((rows, cols), rows + cols, "bf16")
    t = ops.transpose(x)
    rp = -(-rows // 64) * 64
    assert tuple(t.shape) == (cols, rp)
    assert torch.equal(t[:, :rows], x.T) and not t[:, rows:].any()
    g = f32_sum_gate("rowsum", ops.rowsum(t, rows), x.double().sum(dim=0), x.float().sum(dim=0), 256)
    print(f"\n[transpose {rows} x {cols} -> {cols} x {rp}: bit-exact] {g}")
    assert g.ok, str(g)


def _splits(m, n, k):
    """The default split of ops.matmul_nt_splitk and the K range of each split (mavlm_launch_gemm_splitk)."""
    tiles = -(-m // 128) * (n // 128)
    splits = max(1, min(k // 64, -(-512 // tiles)))
    nk = k // 64
    splits = min(splits, nk)
    ksplit = -(-nk // splits) * 64
    splits = -(-k // ksplit)
    return splits, ksplit, k - (splits - 1) * ksplit


@pytest.mark.parametrize("m,n,k", SPLITK_SHAPES, ids=[f"{m}x{n}xK{k}" for m, n, k in SPLITK_SHAPES])
def test_matmul_nt_splitk_m64_vs_fp64(m, n, k):
    """dW = dY^T X through ops.matmul_nt_splitk with its default split count, the operands made as the step makes them
    (ops.transpose of [rows, N] / [rows, K], zero pad to 64 rows): per 256 x 256 tile within GEMM_TILE x the bf16 floor."""
    rows = {32 * P: 32 * P, 1024: 5 * P, R: R}[k]
    dy, x = _randn((rows, m), m + k, "bf16"), _randn((rows, n), n + k + 1, "bf16")
    a, b = ops.transpose(dy), ops.transpose(x)
    assert tuple(a.shape) == (m, k) and tuple(b.shape) == (n, k)
    out = ops.matmul_nt_splitk(a, b)
    worst, ok = gemm_gate(out, dy.double().T @ x.double(), "bf16")
    s, ks, last = _splits(m, n, k)
    print(f"\n[matmul_nt_splitk {m} x {n}, K = {k} ({rows} rows)] {s} splits of {ks}, the last {last}: worst tile {worst:.3f} "
          "x floor")
    assert ok, worst


@pytest.mark.parametrize("m,n,k", MATMUL_NT_SHAPES, ids=[f"{m}x{n}xK{k}" for m, n, k in MATMUL_NT_SHAPES])
def test_matmul_nt_dx_m64_vs_fp64(m, n, k):
    """dX = dY W as the step issues it, ops.matmul_nt(dy, W^T) with W^T from ops.transpose: per 256 x 256 tile within
    GEMM_TILE x the bf16 floor."""
    dy, w = _randn((m, k), m + n + k, "bf16"), _randn((k, n), n + k + 3, "bf16", 1 / 32)
    wT = ops.transpose(w)
    assert tuple(wT.shape) == (n, k)
    worst, ok = gemm_gate(ops.matmul_nt(dy, wT), dy.double() @ w.double(), "bf16")
    print(f"\n[matmul_nt dX {m} x {n}, K = {k}] worst tile {worst:.3f} x floor")
    assert ok, worst


# ------------------------------------------------------------------------------------------------------------ whole step
def _torch_grads(cfg, w, segs, cots, dtype):
    """oracle/torch_path.run_steps on the GPU in `dtype` under autograd, loss sum_t <cache[t], G_t> (accumulated in float64
    for the float64 run, in fp32 otherwise, as the reference's `c.float()`): (loss, {name: gradient as float32 numpy})."""
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    p = TP.params_from(w, dtype, "cuda")
    cache = TP.run_steps(p, cfg, [torch.from_numpy(s).cuda() for s in segs])
    loss = sum((c.to(acc) * torch.from_numpy(g).cuda().to(acc)).sum() for c, g in zip(cache, cots))
    del cache
    g = TP.grads(p, loss)
    out = float(loss.detach())
    del loss, p
    torch.cuda.empty_cache()
    return out, g


@pytest.mark.parametrize("frames", CHUNKINGS, ids=["chunks32-32", "chunks32-5"])
def test_training_step_m64_inside_bf16_envelope(frames):
    """make_projector at hidden 1024, 8 heads, M = 64, depth 2, bf16, train(): BPTT through formation, evolution and formation.
    Every parameter gradient against oracle/torch_path in float64 on the GPU; yardstick: the same restatement under torch bf16
    autograd (the reference's own arithmetic: it runs under torch_dtype=bfloat16), its rel-L2 to float64 per parameter.  Gate
    as test_gradients_inside_reference_bf16_envelope: every parameter <= 1.5 x its envelope, the median <= 1, k_proj.bias
    (true gradient 0) near zero, the loss within 2e-2."""
    w, segs, cots, loss, g, _ = _m64_step(frames)
    torch.cuda.reset_peak_memory_stats()
    loss64, ref = _torch_grads(_CFG, w, segs, cots, torch.float64)
    peak64 = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss16, env = _torch_grads(_CFG, w, segs, cots, torch.bfloat16)
    peak16 = torch.cuda.max_memory_allocated()
    scale = max(np.linalg.norm(v) for v in ref.values())
    rows, ratios, bad = [], [], []
    for name, grad in g.items():
        r, y = ref[TP.PFX + "." + name], env[TP.PFX + "." + name]
        if name.endswith("k_proj.bias"):
            rows.append(f"{name}: |g| / max |ref| = {np.linalg.norm(grad) / scale:.1e}")
            assert np.linalg.norm(grad) <= 2e-3 * scale, name
            continue
        err, e = O.rel_l2(grad, r), O.rel_l2(y, r)
        ratios.append(err / e)
        rows.append(f"{name}: HIP {err:.2e} / envelope {e:.2e} = {err / e:.2f}")
        if err > 1.5 * e:
            bad.append(rows[-1])
    print(f"\n[whole step M=64 chunks {frames}] loss HIP {loss:.6g}, float64 {loss64:.6g}, torch bf16 {loss16:.6g}; "
          f"peak memory float64 {peak64 / 2**30:.1f} GiB, bf16 {peak16 / 2**30:.1f} GiB\n  " + "\n  ".join(rows)
          + f"\n  HIP error / envelope: worst {max(ratios):.2f}, median {np.median(ratios):.2f}")
    assert abs(loss - loss64) <= 2e-2 * abs(loss64)
    assert not bad, bad
    assert np.median(ratios) <= 1.0


def test_gpu_bf16_envelope_matches_the_reference_envelope():
    """The yardstick above is built on the GPU; the one the M = 8 gradient gate uses is the reference's own CPU run
    (env_* in golden/g8_grads_d1024.npz: its bf16-vs-fp32 distance per parameter, on the stored samples).  At that golden's
    shape and seeds the GPU-built envelope (torch bf16 vs float64 on the GPU, the same samples) stays within a factor of 3 of
    the stored one for every parameter, and within a factor of 1.5 at the median."""
    z, meta = load_golden("g8_grads_d1024.npz")
    cfg = O.PathConfig(hidden=meta["hidden"], heads=meta["heads"], mem_tokens=meta["mem_tokens"], depth=meta["depth"])
    w = O.make_weights(cfg, seed=meta["wseed"])
    segs = _segs(cfg, meta["frames"], meta["segseed0"])
    cots = _cotangents(cfg, len(segs), meta["gseed0"], meta["gstd"])
    _, ref = _torch_grads(cfg, w, segs, cots, torch.float64)
    _, y = _torch_grads(cfg, w, segs, cots, torch.bfloat16)
    ratios = {}
    for k in z.files:
        if not k.startswith("env_") or k.endswith("k_proj.bias"):
            continue
        name = TP.PFX + "." + k[4:]
        st = meta["stride"]
        ratios[k[4:]] = O.rel_l2(y[name].reshape(-1)[::st], ref[name].reshape(-1)[::st]) / float(z[k])
    vals = np.array(list(ratios.values()))
    print("\n[bf16 envelope, GPU-built / reference-stored, g8_grads_d1024]\n  "
          + "\n  ".join(f"{n}: {x:.2f}" for n, x in ratios.items())
          + f"\n  min {vals.min():.2f}, median {np.median(vals):.2f}, max {vals.max():.2f}")
    assert len(ratios) == 41
    assert vals.min() >= 1 / 3 and vals.max() <= 3.0, ratios
    assert 1 / 1.5 <= np.median(vals) <= 1.5
