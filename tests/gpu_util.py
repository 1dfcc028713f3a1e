"""Helpers shared by the -m gpu tests: numpy <-> device tensors on the 16-bit grids, oracle weights -> module."""
import math

import numpy as np
import torch

from oracle import memory_path as O

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def to_dev(a: np.ndarray, mode="bf16"):
    """float32 numpy (values already on the grid, or to be rounded) -> 16-bit device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda").to(DT[mode])


def to_np(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def f32_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


def load_oracle_weights(module_root, w: dict, prefix_map=None):
    """Copy oracle weights (reference state-dict names) into a torch module tree (strict on names)."""
    sd = module_root.state_dict()
    used = 0
    for k, v in w.items():
        if k in sd:
            assert tuple(sd[k].shape) == tuple(v.shape), (k, sd[k].shape, v.shape)
            sd[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))
            used += 1
    return used


# ---------------------------------------------------------------------------------------------------------------------------
# Gates against a float64 reference, per unit of work rather than per tensor.  A kernel that is wrong in one 128-row unit out of
# hundreds (a dropped key piece, a misweighted merge) moves a global rel-L2 by little; a per-block rel-L2 sees it.  Every threshold
# is a multiple of a FLOOR computed from the same data: the rel-L2 that an exact result pays for its rounding to the kernel's
# output grid (or, for the backward, for the 16-bit rounding points the kernels document).  Work on torch tensors of any device;
# numpy arrays are taken as well (CPU self-test, tests/test_gates_cpu.py).
ATTN_UNIT, ATTN_WHOLE, LSE2_ATOL = 2.0, 1.5, 1e-4    # forward: per (128-query unit, head), whole tensor, lse2 per row (abs)
GEMM_TILE, GEMM_F32_TILE = 2.0, 2e-5                  # GEMM: 16-bit outputs per 256 x 256 tile (x floor), fp32 outputs (rel-L2)
BWD_BLOCK = 1.5                                       # backward: per (64-row block, head) against the 16-bit-rounding floor
F32_SUM_BLOCK = 8.0                                   # fp32 sums over rows (dgamma, dbeta, bias grads): per block x fp32 floor


def f64(a):
    """torch float64 view of a tensor (same device) or numpy array (CPU)."""
    if isinstance(a, torch.Tensor):
        return a.detach().to(torch.float64)
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def round_to(x, mode):
    """float64 -> the 16-bit grid of `mode` ("bf16" / "fp16", round to nearest even) -> float64."""
    return f64(x).to(DT[mode]).to(torch.float64)


def _block_sq(x, rows, cols):
    R, C = x.shape
    nr, nc = -(-R // rows), -(-C // cols)
    x = torch.nn.functional.pad(x, (0, nc * cols - C, 0, nr * rows - R))
    return x.square().view(nr, rows, nc, cols).sum(dim=(1, 3))


def block_rel_l2(got, ref, rows, cols):
    """rel-L2 of `got` against `ref` per (rows x cols) block of 2-D operands (ragged edge blocks included): [nR, nC] float64.
    A block whose reference is zero counts its error against 1e-300 (zero only if `got` is zero there too)."""
    ref = f64(ref)
    d = f64(got).to(ref.device) - ref
    return torch.sqrt(_block_sq(d, rows, cols) / _block_sq(ref, rows, cols).clamp_min(1e-300))


def rel_l2_t(got, ref):
    ref = f64(ref)
    return float(torch.linalg.vector_norm(f64(got).to(ref.device) - ref) / torch.linalg.vector_norm(ref).clamp_min(1e-300))


class Gate:
    """Result of a floor gate: error / floor per block (`worst`, at block `where`) and over the whole tensor (`whole`)."""

    def __init__(self, name, worst, where, whole, floor, unit, whole_max):
        self.name, self.worst, self.where, self.whole, self.floor = name, worst, where, whole, floor
        self.ok = worst <= unit and (whole_max is None or whole <= whole_max)
        self.limits = (unit, whole_max)

    def __str__(self):
        return (f"{self.name}: worst block {self.worst:.3f} x floor at {self.where}, whole tensor {self.whole:.3f} x floor "
                f"(floor {self.floor:.2e}; limits {self.limits[0]} / {self.limits[1]})")


def floor_gate(name, got, ref, rows, cols, floor, unit, whole_max=None):
    """err(got) / err(floor) per (rows x cols) block and over the whole tensor, both against `ref` (float64).  `floor`: a 16-bit
    mode ("bf16" / "fp16": the floor is ref rounded to that grid) or a tensor (a reference with the kernel's rounding points)."""
    ref = f64(ref)
    fl = round_to(ref, floor) if isinstance(floor, str) else f64(floor).to(ref.device)
    e, f = block_rel_l2(got, ref, rows, cols), block_rel_l2(fl, ref, rows, cols)
    ratio = torch.where(f > 0, e / f.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
    i = int(torch.argmax(ratio))
    gf = rel_l2_t(fl, ref)
    ge = rel_l2_t(got, ref)
    whole = ge / gf if gf > 0 else (0.0 if ge == 0 else float("inf"))
    return Gate(name, float(ratio.view(-1)[i]), divmod(i, ratio.shape[1]), whole, gf, unit, whole_max)


def layernorm_ref64(x, res, gamma, beta, eps):
    """LayerNorm(x + res) * gamma + beta in float64 (biased variance, two passes): x fp32 [rows, D], res 16-bit [rows, D] or
    None, gamma / beta [D]; tensors of any device or numpy arrays."""
    z = f64(x) + (f64(res) if res is not None else 0.0)
    mu = z.mean(dim=1, keepdim=True)
    var = (z - mu).square().mean(dim=1, keepdim=True)
    return (z - mu) / torch.sqrt(var + eps) * f64(gamma) + f64(beta)


LN_ROWS = 4     # rows of a LayerNorm gate block: the rows of one workgroup of the wave-per-row forms (csrc/elementwise.hip)


def layernorm_gate(name, out, ref, mode):
    """Row LayerNorm forward: `out` within BWD_BLOCK x floor per block of LN_ROWS rows, the floor being the float64 `ref` rounded
    once to the output grid (the kernels compute in fp32 and round once: the expected ratio is 1.0)."""
    ref = f64(ref)
    return floor_gate(name, out, ref, LN_ROWS, ref.shape[1], mode, BWD_BLOCK)


# ---------------------------------------------------------------------------------------------------------------------------
# Fused dense + residual + LayerNorm GEMM (EPI_LN of csrc/gemm256.hip and gemm128.hip): inputs whose rows cannot stand in for one
# another, and the gate per LN_ROWS rows x one 256-column tile.  On plain N(0,1) operands the 256-column tile means of a row
# differ by sigma / 16 only, and a row that drops the between-tile term of the merge, or reads a partner's statistics at another
# row, stays under the block limit (tests/test_gates_cpu.py shows it).  Planted: row r of the residual is scaled by s(r) in
# {1/4, 1/2, 1, 2, 4}, and its 256 columns of tile t are shifted by o(r, t) s(r), o a multiple of FUSED_LN_UNIT in [-4, 4].
FUSED_LN_UNIT = 0.5                    # spacing of the tile offsets (exact on both 16-bit grids, as is every offset)
FUSED_LN_DISTANCES = (1, 16, 112, 128, 224, 256)     # neighbour row, 16-row fragment, half tile of each height, tile
_FUSED_LN_PERM = (5, 12, 0, 9, 16, 3, 7, 14, 1, 10, 4, 15, 8, 2, 13, 6, 11)      # a fixed permutation of 0 .. 16


def _hash_idx(i, salt, mod):
    """hashed index in [0, mod) of the int64 tensor i (Knuth's multiplier, two folds; no int64 overflow below i = 2^31)"""
    h = i * 2654435761 + salt * 40503
    return ((h >> 11) ^ (h >> 23) ^ (h >> 5)) % mod


def fused_ln_pattern(M, ntn, device="cpu"):
    """(scale index [M] in 0 .. 4, offset index [M, ntn] in 0 .. 16) of the planted residual: s(r) = 2^(index - 2),
    o(r, t) = (index - 8) x FUSED_LN_UNIT.  The scale is hashed per row.  The offsets of row r are PERM[(r + t step(r)) mod 17]
    with a hashed step(r) in 1 .. 16 and a fixed permutation PERM of 0 .. 16: the (up to 16) tiles of a row all differ (17 is
    prime), so a tile's statistics taken from another tile of the row are wrong ones; and tile 0 holds PERM[r mod 17], which
    differs between rows r and r + d at every d of FUSED_LN_DISTANCES (none is a multiple of 17) - hashed values alone, 5 x 17 of
    them, could not keep the 48 897 rows of a single tile apart from their neighbours."""
    r = torch.arange(M, dtype=torch.int64, device=device)
    s_idx = _hash_idx(r, 1, 5)
    step = 1 + _hash_idx(r, 2, 16)
    t = torch.arange(ntn, dtype=torch.int64, device=device)
    o_idx = torch.tensor(_FUSED_LN_PERM, dtype=torch.int64, device=device)[(r[:, None] + t[None, :] * step[:, None]) % 17]
    return s_idx, o_idx


def fused_ln_inputs(M, N, K, mode, seed, planted=True, device="cuda"):
    """x [M, K], w [N, K], b [N] fp32, res [M, N], gamma [N] fp32, beta [N] fp32 on `device`, distributed as the `_ln_case` of
    tests/test_gpu_batch.py makes them (x and res N(0,1), w uniform within 1 / sqrt(K), b and beta within 0.1, gamma within 0.1
    of 1; 16-bit operands on the grid of `mode`).  `planted`: res = round16(N(0,1) + o(r, t)) s(r), see `fused_ln_pattern`."""
    g = torch.Generator(device=device).manual_seed(seed)
    randn = lambda *shape: torch.randn(shape, generator=g, device=device)
    uni = lambda n, a: (torch.rand((n,), generator=g, device=device) * 2.0 - 1.0) * a
    x = randn(M, K).to(DT[mode])
    w = ((torch.rand((N, K), generator=g, device=device) * 2.0 - 1.0) / math.sqrt(K)).to(DT[mode])
    b = uni(N, 0.1)
    res = randn(M, N)
    if planted:
        s_idx, o_idx = fused_ln_pattern(M, N // 256, device)
        off = ((o_idx - 8).to(torch.float32) * FUSED_LN_UNIT).repeat_interleave(256, dim=1)
        res = (res + off).to(DT[mode]) * torch.exp2((s_idx - 2).to(torch.float32)).to(DT[mode])[:, None]     # (x 2^k: exact)
    else:
        res = res.to(DT[mode])
    return x, w, b, res, 1.0 + uni(N, 0.1), uni(N, 0.1)


def fused_ln_ref64(x, w, b, res, gamma, beta, eps):
    """LayerNorm64(x.double() @ w.double().T + b + res) * gamma + beta on the operands' device: the reference of the fused
    kernel - float64 throughout, never another kernel's output."""
    return layernorm_ref64(x.double() @ w.double().T + b.double(), res, gamma, beta, eps)


def fused_ln_gate(out, ref64, mode):
    """Fused dense + residual + LayerNorm: `out` within BWD_BLOCK x floor per block of LN_ROWS rows x 256 columns (one row group
    of one workgroup's column tile), the floor being `ref64` rounded once to the output grid.  The kernel computes in fp32 and
    rounds once: the expected ratio is 1.0.  `where` = (row block, column tile)."""
    return floor_gate("fused dense+LN", out, ref64, LN_ROWS, 256, mode, BWD_BLOCK)


def attention_gate(ctx, lse2, ref_ctx, ref_lse2, heads, mode):
    """Forward attention: ctx within ATTN_UNIT x floor per (128-query unit, head) and ATTN_WHOLE x floor over the tensor; lse2
    (log2 domain, [H, R]) within LSE2_ATOL of the reference on every row.  Returns (gate, worst lse2 error, passed)."""
    ref_ctx = f64(ref_ctx)
    g = floor_gate("ctx", ctx, ref_ctx, 128, ref_ctx.shape[1] // heads, mode, ATTN_UNIT, ATTN_WHOLE)
    ref_lse2 = f64(ref_lse2)
    lerr = float((f64(lse2).to(ref_lse2.device) - ref_lse2).abs().max())
    return g, lerr, g.ok and lerr <= LSE2_ATOL


def gemm_gate(out, ref, mode=None):
    """GEMM output per 256 x 256 tile: 16-bit outputs (mode "bf16" / "fp16") within GEMM_TILE x floor; fp32 outputs (mode None)
    within GEMM_F32_TILE rel-L2.  Returns (worst ratio or rel-L2, passed)."""
    if mode is not None:
        g = floor_gate("gemm", out, ref, 256, 256, mode, GEMM_TILE)
        return g.worst, g.ok
    worst = float(block_rel_l2(out, ref, 256, 256).max())
    return worst, worst <= GEMM_F32_TILE


def attention_bwd_ref64(q, k, v, do, heads, scale, mode, head_dim, rows=2048, o=None):
    """Gradients of softmax(q k^T scale) v per head of `head_dim` columns in float64, query-blocked by `rows` (works on the
    device of the operands): (exact, rounded), each (dq, dk, dv).  `rounded` takes the rounding points the flash-style backward
    kernels document (attention_bwd.hip, attention_bwd_hd.hip) - the forward output O stored in 16 bits (delta = rowsum(dO o O)),
    P and dS = P o (dP - delta) rounded to 16 bits as the operands of the second products, the scale on the fp32 result, the
    gradients stored in 16 bits - and is the floor of the gate.  `o`: the stored forward output the kernels read (default: the
    exact O rounded to 16 bits).  They differ where the forward's own rounding matters: a nearly one-hot row's O carries the
    16-bit rounding of its dominant probability (taken relative to a stale row maximum, up to 2^8), coherently over the row,
    and dP - delta cancels down to that size."""
    R, S, W = q.shape[0], k.shape[0], heads * head_dim
    z = lambda n: torch.zeros((n, W), device=q.device, dtype=torch.float64)
    ex, rd = [z(R), z(S), z(S)], [z(R), z(S), z(S)]
    rnd = lambda t: round_to(t, mode)
    for h in range(heads):
        sl = slice(h * head_dim, (h + 1) * head_dim)
        kh, vh = k[:, sl].double(), v[:, sl].double()
        for r0 in range(0, R, rows):
            qb, dob = q[r0:r0 + rows, sl].double(), do[r0:r0 + rows, sl].double()
            s = (qb @ kh.T) * scale
            p = torch.exp(s - torch.logsumexp(s, dim=1, keepdim=True))
            oe = p @ vh
            dp = dob @ vh.T
            ds = p * (dp - (dob * oe).sum(dim=1, keepdim=True))
            ob = rnd(oe) if o is None else o[r0:r0 + rows, sl].double()
            ds_r = rnd(p * (dp - (dob * ob).sum(dim=1, keepdim=True)))
            ex[0][r0:r0 + rows, sl] = (ds @ kh) * scale
            rd[0][r0:r0 + rows, sl] = (ds_r @ kh) * scale
            ex[1][:, sl] += (ds.T @ qb) * scale
            rd[1][:, sl] += ds_r.T @ qb
            ex[2][:, sl] += p.T @ dob
            rd[2][:, sl] += rnd(p).T @ dob
        rd[1][:, sl] *= scale
    return ex, [rnd(t) for t in rd]


def f32_sum_gate(name, got, ref, fp32_result, cols):
    """fp32 sums over many rows (LayerNorm dgamma / dbeta, bias gradients): rel-L2 of `got` against the float64 `ref` per block
    of `cols` entries within F32_SUM_BLOCK x an fp32 floor from the same data - per block, the larger of the rel-L2 of a plain
    torch fp32 evaluation of the same sum (`fp32_result`) and of `ref` rounded to fp32 once."""
    ref = f64(ref).reshape(1, -1)
    fl = torch.maximum(block_rel_l2(f64(fp32_result).reshape(1, -1), ref, 1, cols),
                       block_rel_l2(ref.to(torch.float32), ref, 1, cols))
    e = block_rel_l2(f64(got).reshape(1, -1), ref, 1, cols)
    ratio = e / fl.clamp_min(1e-300)
    i = int(torch.argmax(ratio))
    return Gate(name, float(ratio.view(-1)[i]), (0, i), rel_l2_t(got, ref.view(-1)) / max(float(fl.max()), 1e-300),
                float(fl.max()), F32_SUM_BLOCK, None)


# ---------------------------------------------------------------------------------------------------------------------------
# Probability masses: the kernels that SUM softmax probabilities (column sums, frame scores, attention maps) compute in fp32
# throughout, so their floor is an fp32 one, per block of the last dimension.  A query row counted twice or not at all moves a
# block by 1 / R of its value: ~1e-4 at R = 12 544, far under a whole-tensor 1e-3, hundreds of times a block's fp32 floor.
MASS_MIN_TAIL = 8            # a ragged last block of fewer entries is merged into the block before it
F32_ROUND = 2.0 ** -24       # largest relative error of one correct fp32 rounding


def attn_c32(scale):
    """scale x log2 e as the launchers compute it (`a.scale * 1.44269504088896340736f`, one fp32 product): the constant inside the
    kernels' exp2, exactly, as a Python float"""
    return float(np.float32(scale) * np.float32(1.44269504088896340736))


def lse2_offsets(heads, rows):
    """hashed per-(head, row) offsets in [-3, 3], multiples of 1/8 (exactly representable): added to an lse2 that is handed to a
    stand-alone pass, they give every row its own weight, so that a row read at another row's index cannot cancel"""
    i = torch.arange(heads * rows, dtype=torch.int64)
    return ((((i * 2654435761) >> 7) % 49 - 24).to(torch.float32) / 8.0).view(heads, rows)


def _ulp32(x):
    """spacing of fp32 at |x| (float64 tensor)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


def _f32(x):
    """float64 -> fp32 (to nearest even) -> float64"""
    return x.to(torch.float32).double()


def prob_mass_eval(q, k, lse2, heads, head_dim, c, dtype=torch.float64, q_group=None, k_group=None, rows=2048, rounding=None,
                   adds=8):
    """The contract of the probability-mass kernels, evaluated plainly in `dtype` (float64: the reference; float32: the floor):
    p[h][r][s] = exp2(q_h[r] . k_h[s] * c - lse2[h][r]) with the fp32 `lse2` [H, R] and the fp32 constant `c` (scale x log2 e)
    that the kernel was handed, summed over the queries -> [H, S], or, with groups, over `q_group` consecutive rows and
    `k_group` consecutive keys -> [H, ceil(R / q_group), ceil(S / k_group)].  Query-blocked; works on the operands' device.

    `rounding` (float64 only) takes the fp32 rounding points the kernels document - the MFMA accumulator after each 16-column
    step, the product s c, the exponent s c - lse2, the result of exp2, the additions of the sum:
      "emulate"   rounds to nearest at each of them, the sums added in fp32: one realisation of the error, as
                  `attention_bwd_ref64`'s `rounded` (measured on planted rows at 448 columns: the kernels' logits sit within
                  1 .. 4 ulp of float64, either sign, like this emulation's);
      "expected"  returns the reference plus the root-mean-square error those roundings give per output: independent errors,
                  uniform within half an ulp at each point, `adds` additions of the sum.  Its block rel-L2 is the EXPECTED
                  error of a block instead of one draw: the floor of blocks that hold a single exponent (a map cell of one
                  query row, the block of a planted key), where the error of one evaluation says nothing about another's."""
    R, S = q.shape[0], k.shape[0]
    if q_group:
        rows = max(q_group, rows // q_group * q_group)
    ln2 = math.log(2.0)

    def grouped(x, f32_sum=False):
        if f32_sum:
            x = x.to(torch.float32)
        if not q_group:
            return x.sum(0).double() if f32_sum else x.sum(0)
        n, nk = x.shape[0], -(-S // k_group)
        x = torch.nn.functional.pad(x, (0, nk * k_group - S, 0, -(-n // q_group) * q_group - n))
        x = x.view(-1, q_group, nk, k_group).sum(dim=(1, 3))
        return x.double() if f32_sum else x
    out = []
    for h in range(heads):
        sl = slice(h * head_dim, (h + 1) * head_dim)
        kh = k[:, sl].to(dtype)
        acc, var = [], []
        for r0 in range(0, R, rows):
            qb = q[r0:r0 + rows, sl].to(dtype)
            l = lse2[h, r0:r0 + rows, None].to(dtype)
            if rounding is None:
                acc.append(grouped(torch.exp2((qb @ kh.T) * c - l)))
                continue
            s = torch.zeros((qb.shape[0], S), device=q.device, dtype=torch.float64)
            vs = torch.zeros_like(s)
            for j in range(0, head_dim, 16):
                s = s + qb[:, j:j + 16] @ kh[:, j:j + 16].T
                if rounding == "emulate":
                    s = _f32(s)
                else:
                    vs += _ulp32(s) ** 2 / 12.0
            if rounding == "emulate":
                p = _f32(torch.exp2(_f32(_f32(s * c) - l)))
                acc.append(grouped(p, f32_sum=True))
            else:
                t = s * c - l
                vt = c * c * vs + (_ulp32(s * c) ** 2 + _ulp32(t) ** 2) / 12.0
                p = torch.exp2(t)
                acc.append(grouped(p))
                var.append(grouped(p * p * (ln2 * ln2 * vt + 2.0 * F32_ROUND ** 2 / 3.0)))
        if q_group:
            m = torch.cat(acc, 0)
            v = torch.cat(var, 0) if var else None
        else:
            m = acc[0] if len(acc) == 1 else (torch.stack(acc).to(torch.float32).sum(0).double() if rounding == "emulate"
                                               else torch.stack(acc).sum(0))
            v = torch.stack(var).sum(0) if var else None
        if rounding == "expected":
            m = m + torch.sqrt(v + adds * (F32_ROUND * m) ** 2 / 3.0)
        out.append(m)
    return torch.stack(out)


def mass_gate(name, got, ref64, fp32_eval, block):
    """fp32 probability masses whose last dimension is keys, frames or key groups: rel-L2 of `got` against the float64 `ref64`
    per block of `block` consecutive entries of the last dimension, separately for every leading index, within F32_SUM_BLOCK x a
    floor from the same data - per block the largest of the rel-L2 of `fp32_eval` (a plain torch fp32 evaluation of the same
    formula on the same operands), of `ref64` rounded to fp32 once, and of 2^-24 (one correct fp32 rounding: a block that torch
    happens to hit exactly would otherwise have no floor).  A ragged last block of fewer than MASS_MIN_TAIL entries is merged
    into the block before it.  `where` = (flattened leading index, block)."""
    ref = f64(ref64)
    n = ref.shape[-1]
    ref = ref.reshape(-1, n)
    nb = -(-n // block)
    if nb > 1 and 0 < n % block < MASS_MIN_TAIL:
        nb -= 1
    bid = (torch.arange(n, device=ref.device) // block).clamp_max(nb - 1)

    def sq(x):
        return torch.zeros((ref.shape[0], nb), device=ref.device, dtype=torch.float64).index_add_(1, bid, x.square())

    def rel(x):
        return torch.sqrt(sq(f64(x).to(ref.device).reshape(-1, n) - ref) / sq(ref).clamp_min(1e-300))
    fl = torch.maximum(rel(fp32_eval), rel(ref.to(torch.float32))).clamp_min(F32_ROUND)
    ratio = rel(got) / fl
    i = int(torch.argmax(ratio))
    return Gate(name, float(ratio.view(-1)[i]), divmod(i, nb), rel_l2_t(f64(got).reshape(-1, n), ref) / float(fl.max()),
                float(fl.max()), F32_SUM_BLOCK, None)
