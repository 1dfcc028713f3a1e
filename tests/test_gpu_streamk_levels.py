"""-m gpu: every cut level of the attention forward's schedules against torch float64.

Both forwards - attn_fwd3_kernel (head_dim 128, 4- and 8-wave workgroups) and attn_fwd_hd2_kernel (head_dim 448) - run a
schedule that is a pure function of the shape: whole units first, then binary levels whose units are cut into 2^k key ranges
merged by attn_combine_sk_kernel / attn_combine_hd_sk_kernel (one instantiation per k = 1 .. 5), or, on small grids, 2 .. 8 key
planes plus a merge.  The plans launched here are the literals of tests/streamk_cases.py (pinned to the C library on the CPU by
tests/test_plan_mirror_cpu.py): every cut width as a single level, plans of four and five levels, a last level with fewer units
than XCDs, two and three whole rounds before the cut, every split-KV plane count, the frame-score variant and row batches on
multi-level plans.

The reference is torch float64 on the GPU from the same 16-bit operands, query-blocked by 2048 rows (no emulation: it would
re-state the plan).  The gate is `gpu_util.attention_gate`, unchanged: ctx per (128-query unit, head) and over the tensor against
the floor of the same data, lse2 per row.  Every launch is made twice and must repeat bit for bit (static schedule, no atomics).

Inputs: seeded normal operands on the 16-bit grid, then edits that keep them there (copies and powers of two), placed in the
cut units found from the plan, so that the pieces of a cut unit carry very different log-sum-exps:
  late    the last valid row of the unit (the ragged edge where R is no multiple of the unit), scaled by 2, with a copy of the
          unscaled row as a key of the LAST key range: the row's maximum (2 |q_h|^2 / sqrt(hd) ~ 23 against a log-sum-exp of ~10
          over the rest; 42 at 448) arrives in the last piece, which outweighs all others by 2^18 or more;
  hot     the first row: the same in the FIRST key range - a nearly one-hot row whose first piece carries all the mass;
  under   an inner row, scaled by 2^4 (2^3 at 448), with a copy of the unscaled row as a key of a middle range: its lse2 is
          ~200 and the other pieces (lse2 < ~100) enter the merge with weights of 2^-100 or less: nothing is left of them.
          (The rows are scaled, not the keys: a key of 2 x a row gives every OTHER row of the head a logit of twice the usual
          spread, and the few rows that land 4 sigma out put ~half their mass on it with a maximum that grew by less than the
          2^8 rescale threshold - the dominant probability is then no power of two and its rounding to 16 bits, u = 2^-8 in
          bf16, scales the row coherently (the x8 row of test_gpu_ov7b_width.py).  Such a row has half the energy of its
          128-row block: measured 2.5 x its floor, its block - in a WHOLE unit, nothing to do with a merge - 2.014 x.)
          The unit's second range is scaled by 2^-6 (all of it up to four key tiles - the 8-, 16- and 32-way cuts - else its
          first two tiles): near-uniform logits, lse2 ~ 7, so that 2^(lse_piece - lse) underflows to zero for a whole piece.
Key counts: 34 tiles (not divisible by any 2^k: uneven ranges), and 4 / 8 tiles under a 32-way cut (empty pieces).
Measured ratios are printed (-s) and tabulated in tests/README.md."""
import functools

import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from oracle import memory_path as O
from gpu_util import DT, attention_gate, rel_l2_t, round_to, to_dev
import streamk_cases as T

pytestmark = pytest.mark.gpu
TOL = 1e-3                       # the gate of the existing frame-score tests (test_gpu_ops.py, test_gpu_batch.py, test_gpu_frames_lds.py)
LOG2E = 1.4426950408889634
UNDER = {128: 16.0, 448: 8.0, 224: 8.0, 256: 8.0}    # scale of the `under` row: lse2 = scale |q_h|^2 / sqrt(hd) log2 e ...
UNDER_NORM2 = {128: 100.0, 448: 400.0, 224: 240.0, 256: 270.0}   # ... ~ 204 / 218 (185 / 195 at 224 / 256: tests/test_gpu_wide_heads_224_256.py) for the row of a unit with |q_h|^2 nearest to this (mean: hd)


@pytest.fixture(autouse=True)
def _hooks(request, monkeypatch):
    lib = capi.lib()
    request.addfinalizer(lambda: (lib.mavlm_set_attention_streamk_min_tiles(64), lib.mavlm_set_attention_streamk_waves(0),
                                  lib.mavlm_set_frame_entries_lds(1)))

    def set_hooks(min_tiles, waves):
        capi.check(lib.mavlm_set_attention_streamk_min_tiles(min_tiles), "min tiles")
        capi.check(lib.mavlm_set_attention_streamk_waves(waves), "waves")
        monkeypatch.setattr(O, "STREAMK_MIN_TILES", min_tiles)
        monkeypatch.setattr(O, "STREAMK_WAVES", waves)
    with torch.no_grad():
        yield set_hooks


def _geom(kernel):
    """(head_dim, queries per unit, keys per tile)"""
    return {"w8": (128, 256, 64), "w4": (128, 128, 64), "wide": (448, 128, 32), "wide224": (224, 128, 32), "wide256": (256, 128, 32)}[kernel]


def _randn(shape, seed, mode):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda").to(DT[mode])


def _ref64(q, k, v, heads, hd, scale, rows=2048):
    """softmax(q k^T scale) v per head in float64, query-blocked: ctx [R, heads*hd], lse2 [heads, R] (log2 domain), column sums [S]"""
    R, S = q.shape[0], k.shape[0]
    ctx = torch.empty((R, heads * hd), device=q.device, dtype=torch.float64)
    lse2 = torch.empty((heads, R), device=q.device, dtype=torch.float64)
    col = torch.zeros((S,), device=q.device, dtype=torch.float64)
    for h in range(heads):
        sl = slice(h * hd, (h + 1) * hd)
        kh, vh = k[:, sl].double(), v[:, sl].double()
        for r0 in range(0, R, rows):
            s = (q[r0:r0 + rows, sl].double() @ kh.T) * scale
            l = torch.logsumexp(s, dim=1, keepdim=True)
            p = torch.exp(s - l)
            col += p.sum(0)
            ctx[r0:r0 + rows, sl] = p @ vh
            lse2[h, r0:r0 + rows] = l[:, 0] * LOG2E
    return ctx, lse2, col


def _plan_checked(kernel, R, S, H, G, full, levels):
    """the C plan equals the literal (G, whole rounds, levels); returns the cut units [(level, global head, query block, [(tile_lo,
    tile_hi) of the non-empty pieces])], cross-checked with the oracle's cut map"""
    lib = capi.lib()
    hd, QB, KT = _geom(kernel)
    info = (capi.i32 * 4)()
    nqb, nt = -(-R // QB), -(-S // KT)
    pieces = lambda kk: [(a, b) for a, b in (((p * nt) >> kk, ((p + 1) * nt) >> kk) for p in range(1 << kk)) if b > a]
    cuts = []
    if kernel == "wide":
        capi.check(lib.mavlm_attention_hd_plan_info(R, S, H, 448, info), "plan info")
        assert list(info) == [G, full, len(levels), 1], list(info)
        assert O.streamk_plan_wide(R, S, H) == (G, full, levels)
        for lv, (kk, base, n) in enumerate(levels):
            cuts += [(lv, u // nqb, u % nqb, pieces(kk)) for u in range(base, base + n)]
        mirror = O.streamk_split_tiles_wide(R, S, H)
    else:
        capi.check(lib.mavlm_attention_plan(R, S, H, info), "plan")
        assert list(info) == [QB // 32, G, len(levels), 1], list(info)
        assert O.streamk_plan(R, S, H) == (G, QB, full, levels)
        assert lib.mavlm_attention_plan_unit(R, S, H, -1, full - 1, 0) >= 0 and lib.mavlm_attention_plan_unit(R, S, H, -1, full, 0) < 0
        for lv, (kk, base, n) in enumerate(levels):
            assert lib.mavlm_attention_plan_unit(R, S, H, lv, 0, n) < 0
            for b in range(n):
                u = lib.mavlm_attention_plan_unit(R, S, H, lv, 0, b)
                cuts.append((lv, u // nqb, u % nqb, pieces(kk)))
        mirror = O.streamk_split_tiles(R, S, H)[1]
    assert {(h, b): rng for _, h, b, rng in cuts} == mirror and len(mirror) == len(cuts) == nqb * H - full * G
    return cuts


def _plant(qs, ks, heads, cuts, kernel, R, S):
    """The adversarial rows of the module docstring in (at most four per level and head of) the cut units.  qs / ks: per video the
    [R, W] / [S, W] 16-bit operands, edited in place; `cuts` carries global heads (video * heads + head).  Returns the planted
    (video, head, late row, hot row, under row)."""
    hd, QB, KT = _geom(kernel)
    groups = {}
    for lv, hg, qb, rng in cuts:
        groups.setdefault((lv, hg), []).append((qb, rng))
    chosen = []
    for (lv, hg), g in sorted(groups.items()):
        g.sort()
        chosen += [(hg, qb, rng) for qb, rng in {x[0]: x for x in g[:2] + g[-2:]}.values()]
    scaled = set()
    for hg, qb, rng in chosen:                                 # first every scaled-down range, then the planted keys
        b, sl = hg // heads, slice((hg % heads) * hd, (hg % heads + 1) * hd)
        for t in range(rng[1][0], rng[1][1] if rng[1][1] - rng[1][0] <= 4 else rng[1][0] + 2):
            if (hg, t) not in scaled:
                scaled.add((hg, t))
                ks[b][t * KT:(t + 1) * KT, sl] *= 2.0 ** -6
    used, rows = set(), []

    def free_key(hg, keys):
        kj = next(j for j in keys if (hg, j) not in used)
        used.add((hg, kj))
        return kj
    for hg, qb, rng in chosen:
        b, sl = hg // heads, slice((hg % heads) * hd, (hg % heads + 1) * hd)
        q, k = qs[b], ks[b]
        r0, n = qb * QB, min(R, (qb + 1) * QB) - qb * QB
        assert n >= 3 and len(rng) >= 2
        # (the under row: the unit's row whose |q_h|^2 is nearest to UNDER_NORM2 - its lse2 stays below 256, where the fp32 the
        #  kernel returns resolves 1.5e-5, a sixth of LSE2_ATOL)
        d = (q[r0 + 1:r0 + n - 1, sl].float().square().sum(1) - UNDER_NORM2[hd]).abs()
        r_late, r_hot, r_under = r0 + n - 1, r0, r0 + 1 + int(torch.argmin(d))
        lo, hi = rng[-1][0] * KT, min(S, rng[-1][1] * KT)
        mid = rng[len(rng) // 2]
        for r, keys, up in ((r_late, range(hi - 1, lo - 1, -1), 2.0), (r_hot, range(rng[0][0] * KT, rng[0][1] * KT), 2.0),
                            (r_under, range(mid[0] * KT, min(S, mid[1] * KT)), UNDER[hd])):
            k[free_key(hg, keys), sl] = q[r, sl]               # the key is a copy of the row, the ROW is scaled (see above)
            q[r, sl] *= up
        rows.append((b, hg % heads, r_late, r_hot, r_under))
    return rows


def _exact_merge_ratio(q, k, v, h, hd, scale, r0, r1, rng, KT, mode):
    """Diagnostic for a unit that misses its gate: the float64 merge of float64 partials over the unit's key ranges, rounded once
    to 16 bits, against the float64 reference - the floor itself, err / floor = 1.0 if merging is all the schedule does."""
    sl = slice(h * hd, (h + 1) * hd)
    s = (q[r0:r1, sl].double() @ k[:, sl].double().T) * scale
    ref = torch.softmax(s, dim=1) @ v[:, sl].double()
    lp, op = [], []
    for a, b in rng:
        sp = s[:, a * KT:b * KT]
        lp.append(torch.logsumexp(sp, dim=1))
        op.append(torch.softmax(sp, dim=1) @ v[a * KT:b * KT, sl].double())
    lp = torch.stack(lp)
    w = torch.exp(lp - torch.logsumexp(lp, dim=0))
    merged = sum(w[i][:, None] * op[i] for i in range(len(rng)))
    return rel_l2_t(round_to(merged, mode), ref) / max(rel_l2_t(round_to(ref, mode), ref), 1e-300)


def _gate(name, ctx, lse, ref_ctx, ref_lse2, heads, mode, explain=None):
    g, lerr, ok = attention_gate(ctx, lse, ref_ctx, ref_lse2, heads, mode)
    print(f"\n[{name} {mode}] {g}; worst lse2 error {lerr:.2e}")
    if not ok and explain is not None:
        print(f"[{name} {mode}] exact float64 merge of the worst unit's pieces, rounded once: {explain(g.where):.3f} x floor")
    assert ok, (name, str(g), lerr)


def _check_rows(rows, ref_lse2, heads, hd):
    """the planted rows do what they are for: one key dominates (late, hot), every other piece underflows (under)"""
    for b, h, r_late, r_hot, r_under in rows:
        l = ref_lse2[b][h]
        assert float(l[r_late]) > 20.0 and float(l[r_hot]) > 20.0 and float(l[r_under]) > 165.0, (b, h, float(l[r_under]))


def _operands(kernel, R, S, H, mode, seed=500):
    """operands with the adversarial rows, and the float64 reference, of one table case"""
    case = next(c for c in T.STREAMK_CASES if c[:4] == (kernel, R, S, H))
    hd = _geom(kernel)[0]
    cuts = _plan_checked(*case)
    W = H * hd
    q, k, v = _randn((R, W), seed + 1, mode), _randn((S, W), seed + 2, mode), _randn((S, W), seed + 3, mode)
    rows = _plant([q], [k], H, cuts, kernel, R, S)
    scale = ops.attn_scale(hd)
    ref = _ref64(q, k, v, H, hd, scale)
    _check_rows(rows, [ref[1]], H, hd)
    return q, k, v, scale, ref, cuts


def _forward(kernel, q, k, v, H, scale):
    if kernel == "wide":
        return ops.attention(q, k, v, H, want_lse=True, head_dim=448, wide_kernel=True, scale=scale)
    return ops.attention(q, k, v, H, want_lse=True, scale=scale)


def _multi(c):
    return len(c[6]) > 1


_LEVEL_PARAMS = [pytest.param(c, "bf16", id=T.case_id(c) + "-bf16") for c in T.STREAMK_CASES] + \
                [pytest.param(c, "fp16", id=T.case_id(c) + "-fp16") for c in T.STREAMK_CASES if _multi(c)]


@pytest.mark.parametrize("case,mode", _LEVEL_PARAMS)
def test_forward_on_every_cut_level_vs_fp64(case, mode, _hooks):
    """Every plan of the table through `ops.attention`: the exact level list, the float64 gates, the same bits twice."""
    kernel, R, S, H, G, full, levels = case
    _hooks(T.MIN_TILES, T.WAVES[kernel])
    hd, QB, KT = _geom(kernel)
    q, k, v, scale, (ref_ctx, ref_lse2, _), cuts = _operands(kernel, R, S, H, mode)
    ctx, lse = _forward(kernel, q, k, v, H, scale)
    again, lse_again = _forward(kernel, q, k, v, H, scale)
    assert torch.equal(again, ctx) and torch.equal(lse_again, lse)
    by_unit = {(h, b): rng for _, h, b, rng in cuts}

    def explain(where):                                        # (128-query block, head) of the gate -> the plan's unit
        rb, h = where
        rng = by_unit.get((h, rb * 128 // QB))
        return float("nan") if rng is None else _exact_merge_ratio(q, k, v, h, hd, scale, rb * 128, min(R, rb * 128 + 128), rng, KT, mode)
    _gate(f"{T.case_id(case)} full {full} levels {levels}", ctx, lse, ref_ctx, ref_lse2, H, mode, explain)


# --------------------------------------------------------------------------------------------------------------- frame scores
_FRAME_PLANS = [("w8", 20729), ("w4", 12155), ("w4", 18549)]   # two levels behind two whole rounds; five levels; full = 2 on 4 waves
_FRAME_PARAMS = [pytest.param(kn, R, "bf16", id=f"{kn}-R{R}-bf16") for kn, R in _FRAME_PLANS] + \
                [pytest.param("w4", 12155, "fp16", id="w4-R12155-fp16")]


@functools.lru_cache(maxsize=1)
def _frame_operands(kernel, R, F, P, mode):
    """operands and float64 reference of one frame-score shape: computed once, shared by the two entry forms, never modified"""
    case = next(c for c in T.STREAMK_CASES if c[:2] == (kernel, R))
    H, S = case[3], F * P
    cuts = _plan_checked(kernel, R, S, H, *case[4:])           # (min tiles 1: the plan does not depend on S)
    q, k, v = _randn((R, H * 128), 601, mode), _randn((S, H * 128), 602, mode), _randn((S, H * 128), 603, mode)
    rows = _plant([q], [k], H, cuts, kernel, R, S)
    scale = ops.attn_scale(128)
    ref = _ref64(q, k, v, H, 128, scale)
    _check_rows(rows, [ref[1]], H, 128)
    return q, k, v, H, scale, ref


@pytest.mark.parametrize("lds", [1, 0], ids=["lds", "scratch"])
@pytest.mark.parametrize("P,F", [(64, 31), (196, 11)], ids=["P64xF31", "P196xF11"])
@pytest.mark.parametrize("kernel,R,mode", _FRAME_PARAMS)
def test_frame_scores_across_levels_vs_fp64(kernel, R, mode, P, F, lds, _hooks):
    """`ops.attention_frames` on multi-level plans - the frame entries of cut units are merged across levels by the combine
    kernel: P = 64 x 31 frames (31 key tiles: every frame boundary at a tile end, one empty piece under the 32-way cut) and
    P = 196 x 11 frames (34 tiles: boundaries inside tiles and inside pieces), entries of whole units in LDS and through the
    scratch.  Scores against float64 column sums averaged per frame, ctx / lse2 bit-identical to the forward without scores on
    the same schedule and inside the float64 gates, the same bits twice."""
    lib = capi.lib()
    _hooks(T.MIN_TILES, T.WAVES[kernel])
    capi.check(lib.mavlm_set_frame_entries_lds(lds), "hook")
    q, k, v, H, scale, (ref_ctx, ref_lse2, col) = _frame_operands(kernel, R, F, P, mode)
    S = F * P
    assert lib.mavlm_attention_frames_ws_floats(R, S, H, P) > 0
    ctx, lse, scores = ops.attention_frames(q, k, v, H, P, want_lse=True, scale=scale)
    again = ops.attention_frames(q, k, v, H, P, want_lse=True, scale=scale)
    assert torch.equal(again[0], ctx) and torch.equal(again[1], lse) and torch.equal(again[2], scores)
    plain, lse_p = ops.attention(q, k, v, H, want_lse=True, scale=scale)
    assert torch.equal(ctx, plain) and torch.equal(lse, lse_p)
    _gate(f"frames {kernel}-R{R} P{P}xF{F} {'lds' if lds else 'scratch'}", ctx, lse, ref_ctx, ref_lse2, H, mode)
    err = rel_l2_t(scores, col.view(F, P).mean(1))
    print(f"frame scores vs float64 column sums: rel-L2 {err:.2e}; sum x P / (H R) = {float(scores.sum()) * P / (H * R):.6f}")
    assert err < TOL and abs(float(scores.sum()) * P - H * R) < 1e-3 * H * R


def test_wide_head_frame_scores_on_a_multi_level_plan():
    """head_dim 448: the frame scores ride on the last formation layer's forward (tile entries, `attn_fwd_hd2_kernel<.., FT = 1>`) -
    the route of test_gpu_path.py::test_wide_head_frame_scores_ride_on_the_forward, here at 38 memory tokens over a 21-frame
    chunk, where that forward runs a four-level plan under the default hooks: against the column-sum pass on the same inputs the
    memory is bit-identical and the scores agree to the rounding of their 16-bit storage.  (A kernel trace of this step in the
    default mode shows the FT = 1 forward, attn_combine_hd_sk_kernel and frame_tiles_kernel, and no column-sum kernel; the
    library's launch counters do not tell the two routes of the wide heads apart, so the test cannot assert it.)"""
    from test_gpu_path import make_projector
    M, F, P = 38, 21, 196
    info = (capi.i32 * 4)()
    lib = capi.lib()
    capi.check(lib.mavlm_attention_hd_plan_info(M * P, F * P, 8, 448, info), "plan info")
    assert list(info) == [256, 1, 4, 1]
    assert O.streamk_plan_wide(M * P, F * P, 8) == (256, 1, [(1, 256, 128), (2, 384, 64), (4, 448, 16), (5, 464, 8)])
    cfg = O.PathConfig(hidden=3584, heads=8, mem_tokens=M, depth=2)
    proj = make_projector(cfg, O.make_weights(cfg, seed=79))
    seg = to_dev(O.bf16_round(O.hash_normal_like((F, P, 3584), 7900)))
    got = {}
    try:
        for fs_mode in (1, 0):
            capi.check(lib.mavlm_set_frame_score_mode(fs_mode), "mode")
            proj.memory_cache = []
            cache, scores = proj(seg)
            got[fs_mode] = (cache[-1].clone(), scores[-1].clone())
    finally:
        lib.mavlm_set_frame_score_mode(1)
    assert torch.equal(got[1][0], got[0][0])
    err = rel_l2_t(got[1][1], got[0][1])
    print(f"\n[wide frame scores, four-level plan] fused vs column-sum pass: rel-L2 {err:.2e}; sum {float(got[1][1].float().sum()):.3f}")
    assert got[1][1].shape == got[0][1].shape and err < 5e-3
    assert abs(float(got[1][1].float().sum()) - 8 * M) < 2e-2 * 8 * M


# ----------------------------------------------------------------------------------------------------------------- row batches
@pytest.mark.parametrize("case", T.BATCH_CASES, ids=[f"{c[0]}-nb{c[1]}-R{c[2]}-H{c[4]}" for c in T.BATCH_CASES])
def test_row_batch_on_multi_level_plans_vs_fp64(case, _hooks):
    """`ops.attention_batch` with different Q / K / V per video on a multi-level plan laid over the (video, head) pairs of all
    videos, every video against its own float64 reference.  head_dim 128 deals cut units to every video (XCD-affine order);
    the position order of the wide kernel cuts the tail of the head-major order: the last video at nb = 2, the last two at
    nb = 3 (tests/test_plan_mirror_cpu.py asserts which)."""
    kernel, nb, R, S, H, G, full, levels = case
    mode = "bf16"
    _hooks(T.MIN_TILES, 0)
    hd, QB, KT = _geom(kernel)
    heads = H // nb
    cuts = _plan_checked(kernel, R, S, H, G, full, levels)
    assert len({hg // heads for _, hg, _, _ in cuts}) >= 2 or (kernel == "wide" and nb == 2)
    W = heads * hd
    q, k, v = _randn((nb * R, W), 701, mode), _randn((nb, S, W), 702, mode), _randn((nb, S, W), 703, mode)
    rows = _plant([q[b * R:(b + 1) * R] for b in range(nb)], [k[b] for b in range(nb)], heads, cuts, kernel, R, S)
    scale = ops.attn_scale(hd)
    ctx, lse = ops.attention_batch(q, k, v, heads, nb, want_lse=True, head_dim=hd, scale=scale)
    again, lse_again = ops.attention_batch(q, k, v, heads, nb, want_lse=True, head_dim=hd, scale=scale)
    assert torch.equal(again, ctx) and torch.equal(lse_again, lse)
    refs = [_ref64(q[b * R:(b + 1) * R], k[b], v[b], heads, hd, scale) for b in range(nb)]
    _check_rows(rows, [r[1] for r in refs], heads, hd)
    for b in range(nb):
        _gate(f"batch {kernel} nb {nb} R{R} video {b} levels {levels}", ctx[b * R:(b + 1) * R], lse[b * heads:(b + 1) * heads],
              refs[b][0], refs[b][1], heads, mode)


# -------------------------------------------------------------------------------------------------------------------- split-KV
_SPLIT_PARAMS = [pytest.param(128, R, S, H, n, id=f"hd128-R{R}-S{S}-H{H}-{n}planes") for R, S, H, n, _ in T.SPLIT_CASES if n] + \
                [pytest.param(448, R, S, H, n, id=f"hd448-R{R}-S{S}-H{H}-{n}planes") for R, S, H, _, n in T.SPLIT_CASES if n]


@pytest.mark.parametrize("hd,R,S,H,planes", _SPLIT_PARAMS)
def test_split_kv_every_plane_count_vs_fp64(hd, R, S, H, planes, _hooks):
    """The small grids' key planes, 2 .. 8 at head_dim 128 and 2 .. 7 at 448, under the default hooks: every (128-query block,
    head) is cut into `planes` ranges of tiles-per-plane key tiles (the last one shorter and ragged) - the same adversarial rows,
    the same gates."""
    lib = capi.lib()
    _hooks(64, 0)
    mode = "bf16"
    kernel = "w4" if hd == 128 else "wide"                     # (the geometry of the units: 128 queries, 64- / 32-key tiles)
    KT = _geom(kernel)[2]
    info = (capi.i32 * 4)()
    if hd == 128:
        capi.check(lib.mavlm_attention_plan(R, S, H, info), "plan")
        ns, tps = O.split_plan(R, S, H)
        assert info[1] == 0 and lib.mavlm_attention_ws_floats(R, S, H) == ns * (R * H * 128 + H * R)
    else:
        capi.check(lib.mavlm_attention_hd_plan_info(R, S, H, 448, info), "plan info")
        ns, tps = O.split_plan_wide(R, S, H)
        assert info[0] == 0 and lib.mavlm_attention_hd_ws_floats(R, S, H, 448) == ns * (R * H * 448 + H * R)
    assert info[3] == planes == ns
    nt = -(-S // KT)
    rng = [(p * tps, min(nt, (p + 1) * tps)) for p in range(ns)]
    cuts = [(0, h, b, rng) for h in range(H) for b in range(-(-R // 128))]
    q, k, v = _randn((R, H * hd), 801, mode), _randn((S, H * hd), 802, mode), _randn((S, H * hd), 803, mode)
    rows = _plant([q], [k], H, cuts, kernel, R, S)
    scale = ops.attn_scale(hd)
    ctx, lse = _forward(kernel, q, k, v, H, scale)
    again, lse_again = _forward(kernel, q, k, v, H, scale)
    assert torch.equal(again, ctx) and torch.equal(lse_again, lse)
    ref_ctx, ref_lse2, _ = _ref64(q, k, v, H, hd, scale)
    _check_rows(rows, [ref_lse2], H, hd)
    _gate(f"split-KV hd{hd} R{R} S{S} H{H}: {ns} planes of {tps} tiles", ctx, lse, ref_ctx, ref_lse2, H, mode,
          lambda w: _exact_merge_ratio(q, k, v, w[1], hd, scale, w[0] * 128, min(R, w[0] * 128 + 128), rng, KT, mode))
