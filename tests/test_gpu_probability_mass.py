"""-m gpu: the kernels that SUM softmax probabilities - column sums, frame scores, attention maps - against float64 per block.

Every other kernel family is held to a few times a rounding floor per unit of work; these were held to a whole-tensor 1e-3 although
they compute in fp32 throughout.  Their outputs steer a discrete decision (which frames the FIFO evicts or samples) and their
schedules have seams - pieces of a unit in separate planes, workgroups that start and end inside a unit - where a query row can
be counted twice or not at all: ~1e-4 of a column sum at the workload's 12 544 rows.  `gpu_util.mass_gate` sees one such row from a
block of 32 keys (one wave of attn_colsum3_kernel), one frame or one key group: 8 x an fp32 floor taken from the same data
(tests/test_gates_cpu.py plants the defects).

Reference: the kernels' own contract in float64 on the GPU, sum_q exp2(s c - lse2[h][q]), with the fp32 lse2 tensor the kernel
read (`gpu_util.prob_mass_eval`) - for the fused forms the lse2 the launch returned.  No log-sum-exp is recomputed: lse2 itself
stays under LSE2_ATOL where it is tested today, and this gate measures the sums alone.

Stand-alone passes take lse2 as an INPUT: they are handed the float64 log-sum-exp rounded to fp32 plus a hashed offset in [-3, 3]
per row (`gpu_util.lse2_offsets`), so every row carries its own weight and a misindexed lse2 cannot cancel; the tensor lies in a
larger buffer whose entries behind [H, R] hold -30 (a read past the end adds 2^30).

Operands, bf16 and fp16: plain N(0,1) on the grid, and the same with planted rows - a row scaled by 8 with an unscaled copy as a
key (lse2 ~ 130 at 128 columns, ~ 245 at 448), a row scaled by 2 whose copy is the LAST free key (its maximum arrives in the last
key range), one whose copy is the FIRST free key (nearly one-hot from the start) - in turn at: the first and last row of a query
tile, the last valid row, and the two rows either side of every seam of the case's plan (tests/mass_cases.py; for the fused
forward: the first and last row of every cut unit).  The first planted keys are the last key and, where S is ragged against
the 128-key blocks, the first key of the ragged block.  Every launch runs twice and must repeat bit for bit; results go into
buffers guarded by a sentinel.  Which kernels ran is read from the launch counters (`mavlm_prof_enable`).

Two kinds of case have blocks that hold a single exponent, where ONE torch fp32 evaluation is no floor (`_single_exponent`; both
ratios are printed and tabulated): a map cell of one query row, and the block of a planted key at 448 columns.  Their floor is
the expected magnitude of the kernels' fp32 rounding points (`prob_mass_eval(rounding="expected")`), about the size of a
correct evaluation's error and under MAX_FLOOR like every floor here; the limit stays F32_SUM_BLOCK.

The frame-tile form (FR = 2) and the head-448 frame entries (frame_tiles_kernel) have no operator export: tests/test_gpu_path.py
ties them to the column-sum pass bit for bit / to 16-bit rounding.  `k_rot` of the maps is not reachable from Python: the map
tests of tests/test_gpu_attention_maps.py cover it through the step.  Measured ratios: tests/README.md."""
import ctypes
import functools
import math

import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from gpu_util import DT, attn_c32, lse2_offsets, mass_gate, prob_mass_eval
import mass_cases as T

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
BIG = 3.0e4                      # rows between the videos of a K buffer (test_gpu_colsum_batch.py)
LN2 = math.log(2.0)
MAX_FLOOR = 1e-4                 # a block floor above this would hide one row at R = 12 544
MODES = ["bf16", "fp16"]
KINDS = ["plain", "planted"]


@pytest.fixture(autouse=True)
def _hooks(request):
    lib = capi.lib()
    request.addfinalizer(lambda: (lib.mavlm_set_attention_impl(0), lib.mavlm_set_attention_colsum_wgs(0),
                                  lib.mavlm_set_attention_streamk_min_tiles(64), lib.mavlm_set_attention_streamk_waves(0),
                                  lib.mavlm_set_frame_entries_lds(1), lib.mavlm_prof_enable(0)))
    with torch.no_grad():
        yield


# --------------------------------------------------------------------------------------------------------------------- helpers
def _randn(shape, seed, mode):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda").to(DT[mode])


def _plant(q, k, rows, big=8.0):
    """the planted rows of the module docstring, in place, at `rows` of q [R, W] with their keys in k [S, W] (all heads at once:
    the key is a copy of the whole row, the ROW is scaled - powers of two keep it on the grid; `big`: the scale of the first
    kind of row).  Returns {row: key}."""
    R, S = q.shape[0], k.shape[0]
    rows = sorted({r for r in rows if 0 <= r < R})
    assert len(rows) <= S // 3, (len(rows), S)
    ragged = [S // 128 * 128] if S % 128 and S > 128 else []
    order = {"late": list(range(S - 1, -1, -1)), "hot": list(range(S)), "x8": ragged + list(range(S // 2, S)) + list(range(S // 2))}
    used, keys = set(), {}
    for i, r in enumerate(rows):
        kind = ("late", "x8", "hot")[i % 3]
        key = next(j for j in order[kind] if j not in used)
        used.add(key)
        keys[r] = key
        k[key] = q[r]
        q[r] *= big if kind == "x8" else 2.0
    return keys


def _tile_rows(R, tile, seam_tiles=()):
    """first and last row of a query tile (the second one where there is one), the last valid row, both rows at every seam"""
    rows = {tile, 2 * tile - 1} if R >= 2 * tile else {0, min(tile, R) - 1}
    rows.add(R - 1)
    for t in seam_tiles:
        rows |= {t * tile - 1, t * tile}
    return rows


def _lse_input(q, k, H, hd, c):
    """the lse2 a stand-alone pass is handed: float64 log-sum-exp (log2 domain) rounded to fp32 + the hashed offsets, [H, R] at the
    start of a larger buffer that holds -30 behind it"""
    R = q.shape[0]
    big = torch.full((H * R + 4096,), -30.0, device="cuda", dtype=torch.float32)
    lse = big[:H * R].view(H, R)
    for h in range(H):
        sl = slice(h * hd, (h + 1) * hd)
        kh = k[:, sl].double()
        for r0 in range(0, R, 2048):
            s = (q[r0:r0 + 2048, sl].double() @ kh.T) * (c * LN2)
            lse[h, r0:r0 + 2048] = (torch.logsumexp(s, dim=1) / LN2).float()
    lse += lse2_offsets(H, R).to("cuda")
    return lse


def _guarded(n, tail=256):
    """fp32 buffer of n floats + a tail, all sentinel"""
    return torch.full((n + tail,), SENTINEL, device="cuda", dtype=torch.float32)


def _intact(buf, start):
    return bool((buf[start:] == SENTINEL).all())


def _counted(fn):
    """fn() with the launch counters on: (result, {kernel kind: launches})"""
    lib = capi.lib()
    nk = len(capi.KERNEL_KINDS)
    torch.cuda.synchronize()
    lib.mavlm_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        ms, fl, by = (ctypes.c_double * nk)(), (ctypes.c_double * nk)(), (ctypes.c_double * nk)()
        ln = (ctypes.c_int64 * nk)()
        capi.check(lib.mavlm_prof_read(ms, ln, fl, by, nk), "mavlm_prof_read")
    finally:
        lib.mavlm_prof_enable(0)
    return out, {kind: int(ln[i]) for i, kind in enumerate(capi.KERNEL_KINDS) if ln[i]}


def _gate(name, got, ref64, f32, block, expected=None):
    """the gate of one result.  `expected` (see `_single_exponent`): the form's floor is the expected magnitude of the fp32
    rounding points instead of torch's one draw; the ratio against the torch fp32 evaluation is printed next to it.  Whichever
    floor is used stays under MAX_FLOOR."""
    g = mass_gate(name, got, ref64, f32, block)
    print(f"\n[mass] {g}")
    if expected is not None:
        g = mass_gate(name + " / expected rounding", got, ref64, expected, block)
        print(f"[mass] {g}")
    assert g.floor < MAX_FLOOR, str(g)
    assert g.ok, str(g)
    return g


def _single_exponent(hd, kind, q_group=None):
    """Cases with blocks that hold ONE exponent, so that the error of one fp32 evaluation is no floor for another's (measured,
    tests/README.md): a map cell of one query row - four probabilities of one row; where torch happens to land within 2^-24 any
    other correct evaluation sits up to 14 x above it, on plain operands too - and the block of a planted key at 448 columns,
    one probability whose logit of ~3600 went through 28 accumulator roundings of 2.4e-4: the kernels' logits and torch's are
    both a few ulp from float64, independently, and where torch's error is 3e-5 of the probability the kernel's 3e-4 reads as
    12 .. 34 x (torch's bf16 draw, 1.3e-4, is itself above MAX_FLOOR).  Their floor is `prob_mass_eval(rounding="expected")`."""
    return q_group == 1 or (hd == 448 and kind == "planted")


def _scale(hd):
    return ops.attn_scale(hd)


# ------------------------------------------------------------------------------------------------- column sums, head_dim 128
@functools.lru_cache(maxsize=4)
def _colsum_setup(R, S, H, mode, kind):
    """operands, the lse2 input and both evaluations of one table shape: computed once, shared by every plan and kernel of the
    shape, never modified.  Planted rows: at the seams of EVERY plan the table lists for the shape."""
    hd = 128
    q, k = _randn((R, H * hd), 4100 + R, mode), _randn((S, H * hd), 4200 + S, mode)
    if kind == "planted":
        seams = sorted({t for c in T.COLSUM_CASES if c[:3] == (R, S, H) for t in T.colsum_seam_tiles(R, S, H, c[4])})
        _plant(q, k, _tile_rows(R, 64, seams))
    c = attn_c32(_scale(hd))
    lse = _lse_input(q, k, H, hd, c)
    return q, k, lse, prob_mass_eval(q, k, lse, H, hd, c), prob_mass_eval(q, k, lse, H, hd, c, torch.float32)


def _launch_colsum(q, k, lse, H, planes):
    """`mavlm_attention_colsum` into a guarded buffer: [H, S]; nothing behind the planes the plan uses is written"""
    lib = capi.lib()
    R, S = q.shape[0], k.shape[0]
    per = int(lib.mavlm_attention_colsum_floats(R, S, H))
    assert per >= planes * H * S
    buf = _guarded(per)
    capi.check(lib.mavlm_attention_colsum(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), lse.data_ptr(), buf.data_ptr(), per,
                                          R, S, H, _scale(128), ops.dtype_code(q.dtype), ops.stream_ptr()), "mavlm_attention_colsum")
    torch.cuda.synchronize()
    assert _intact(buf, planes * H * S), "written behind the planes"
    return buf[:H * S].view(H, S).clone()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", T.COLSUM_CASES, ids=T.case_id)
def test_column_sums_on_every_plan_of_the_table(case, mode, kind):
    """attn_colsum3_kernel (impl 3) + colsum_planes_reduce_kernel on the plan of the table row, and, once per shape,
    attn_colsum_kernel (impl 2: one plane, one workgroup per unit)"""
    R, S, H, wgs, G, planes = case
    lib = capi.lib()
    q, k, lse, ref, f32 = _colsum_setup(R, S, H, mode, kind)
    info = (ctypes.c_int32 * 2)()
    for impl in ([3, 2] if wgs == 0 else [3]):
        capi.check(lib.mavlm_set_attention_impl(impl), "impl")
        capi.check(lib.mavlm_set_attention_colsum_wgs(wgs), "colsum wgs")
        capi.check(lib.mavlm_attention_colsum_plan(R, S, H, info), "colsum plan")
        want = (G, planes) if impl == 3 else (G, 1)
        assert (info[0], info[1]) == want, (impl, list(info))
        got, ln = _counted(lambda: _launch_colsum(q, k, lse, H, want[1]))
        assert ln == ({"attention_colsum": 1, "misc": 1} if want[1] > 1 else {"attention_colsum": 1}), (impl, ln)
        assert torch.equal(_launch_colsum(q, k, lse, H, want[1]), got)
        _gate(f"colsum impl {impl} R{R} S{S} H{H} wgs {wgs} (G {G}, {want[1]} planes) {mode} {kind}", got, ref, f32, 32)


# ---------------------------------------------------------------------------------------------------------- wide column sums
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hd,R,S,H", T.WIDE_CASES, ids=lambda v: str(v))
def test_wide_column_sums(hd, R, S, H, mode, kind):
    """attn_colsum_hd_kernel<T, 448> and <T, 128> (`wide_kernel=True`): 32-row tiles, R ragged against them"""
    lib = capi.lib()
    q, k = _randn((R, H * hd), 4300 + R, mode), _randn((S, H * hd), 4400 + S, mode)
    if kind == "planted":
        _plant(q, k, _tile_rows(R, 32))
    scale = _scale(hd)
    c = attn_c32(scale)
    lse = _lse_input(q, k, H, hd, c)

    def launch():
        buf = _guarded(H * S)
        capi.check(lib.mavlm_attention_colsum_hd(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), lse.data_ptr(), buf.data_ptr(),
                                                 R, S, H, hd, scale, ops.dtype_code(q.dtype), ops.stream_ptr()), "mavlm_attention_colsum_hd")
        torch.cuda.synchronize()
        assert _intact(buf, H * S)
        return buf[:H * S].view(H, S).clone()
    got = launch()                                                # (this export has one kernel and no launch counter)
    assert torch.equal(launch(), got)
    assert torch.equal(ops.attention_colsum(q, k, lse, H, head_dim=hd, wide_kernel=True, scale=scale), got)
    exp = prob_mass_eval(q, k, lse, H, hd, c, rounding="expected", adds=R // 32 + 5) if _single_exponent(hd, kind) else None
    _gate(f"colsum wide hd{hd} R{R} S{S} H{H} {mode} {kind}", got, prob_mass_eval(q, k, lse, H, hd, c),
          prob_mass_eval(q, k, lse, H, hd, c, torch.float32), 32, exp)


# ---------------------------------------------------------------------------------------------------------------- row batches
def _batch_operands(hw, nb, H, R, key_counts, mode, kind, seams, seed):
    """stacked Q [nb R, W]; K per video as column slices of one wider buffer whose other entries hold 3e4 (rows between two
    videos included); every video its own data, planted rows and lse2 input.  Returns q, [k_b], lse [nb H, R], the buffer."""
    W = H * hw
    q = _randn((nb * R, W), seed, mode)
    gap = 5
    buf = torch.full((sum(key_counts) + gap * nb, W + 64), BIG, device="cuda", dtype=DT[mode])
    ks, at = [], 0
    for b, S in enumerate(key_counts):
        kb = buf[at:at + S, 32:32 + W]
        kb.copy_(_randn((S, W), seed + 1 + b, mode))
        if kind == "planted":
            _plant(q[b * R:(b + 1) * R], kb, _tile_rows(R, 64 if hw == 128 else 32, seams[b]))
        ks.append(kb)
        at += S + gap
    c = attn_c32(_scale(hw))
    big = torch.full((nb * H * R + 4096,), -30.0, device="cuda", dtype=torch.float32)
    lse = big[:nb * H * R].view(nb * H, R)
    for b in range(nb):
        lse[b * H:(b + 1) * H] = _lse_input(q[b * R:(b + 1) * R], ks[b], H, hw, c)
    return q, ks, lse, buf


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw,nb,H,R,S", T.BATCH_CASES, ids=lambda v: str(v))
def test_batched_column_sums(hw, nb, H, R, S, mode, kind):
    """attn_colsum3_kernel<T, NB> + colsum_planes_reduce_kernel (grid y = video) and the row batch of attn_colsum_hd_kernel"""
    lib = capi.lib()
    G, planes = T.BATCH_PLANS[(R, S, H)] if hw == 128 else (0, 1)
    seams = T.colsum_seam_tiles(R, S, H, G) if hw == 128 else ()
    q, ks, lse, kbuf = _batch_operands(hw, nb, H, R, [S] * nb, mode, kind, [seams] * nb, 4500 + R)
    k = torch.as_strided(kbuf, (nb, S, H * hw), ((S + 5) * kbuf.stride(0), kbuf.stride(0), 1), 32)
    assert all(k[b].data_ptr() == ks[b].data_ptr() for b in range(nb))
    scale = _scale(hw)
    c = attn_c32(scale)
    per = int(lib.mavlm_attention_colsum_floats(R, S, H))
    assert int(lib.mavlm_attention_colsum_batch_floats(R, S, H, nb)) == nb * per

    def launch():
        buf = _guarded(nb * per)
        capi.check(lib.mavlm_attention_colsum_batch(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0), lse.data_ptr(),
                                                    buf.data_ptr(), nb * per, R, S, H, nb, hw, scale, ops.dtype_code(q.dtype),
                                                    ops.stream_ptr()), "mavlm_attention_colsum_batch")
        torch.cuda.synchronize()
        body = buf[:nb * per].view(nb, per)
        assert bool((body[:, planes * H * S:] == SENTINEL).all()) and _intact(buf, nb * per)
        return body[:, :H * S].reshape(nb, H, S).clone()
    got, ln = _counted(launch)
    # (the wide kernel's launcher keeps no counter: head width 448 is asserted through the export's argument alone)
    assert ln == ({} if hw == 448 else {"attention_colsum": 1, "misc": 1} if planes > 1 else {"attention_colsum": 1}), ln
    assert torch.equal(launch(), got)
    for b in range(nb):
        qb, lb = q[b * R:(b + 1) * R], lse[b * H:(b + 1) * H]
        exp = prob_mass_eval(qb, ks[b], lb, H, hw, c, rounding="expected", adds=R // 32 + 5) if _single_exponent(hw, kind) else None
        _gate(f"colsum batch hd{hw} nb{nb} R{R} S{S} H{H} video {b} ({planes} planes) {mode} {kind}", got[b],
              prob_mass_eval(qb, ks[b], lb, H, hw, c), prob_mass_eval(qb, ks[b], lb, H, hw, c, torch.float32), 32, exp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_variable_length_batched_column_sums(mode, kind):
    """attn_colsum3_kernel<T, NB, VL> + colsum_planes_reduce_vl_kernel: every video its own key count, G and plane count - one
    multi-plane, one single-plane, one shorter than a key block"""
    lib = capi.lib()
    R, H, keys, plans = T.VARLEN_CASE
    nb = len(keys)
    seams = [T.colsum_seam_tiles(R, s, H, g) for s, (g, _) in zip(keys, plans)]
    q, ks, lse, kbuf = _batch_operands(128, nb, H, R, keys, mode, kind, seams, 4600)
    scale = _scale(128)
    c = attn_c32(scale)
    # packed keys (the operator's layout): the videos back to back, still column slices of a wider buffer
    packed = torch.full((sum(keys), H * 128 + 64), BIG, device="cuda", dtype=DT[mode])
    k = packed[:, 32:32 + H * 128]
    k.copy_(torch.cat(ks))
    per = [int(lib.mavlm_attention_colsum_floats(R, s, H)) for s in keys]
    offs = [sum(keys[:b]) * k.stride(0) for b in range(nb)]

    def launch():
        buf = _guarded(sum(per))
        capi.check(lib.mavlm_attention_colsum_batch_varlen(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0),
                                                           (ctypes.c_int64 * nb)(*offs), lse.data_ptr(), buf.data_ptr(), sum(per), R,
                                                           (ctypes.c_int32 * nb)(*keys), H, nb, 128, scale, ops.dtype_code(q.dtype),
                                                           ops.stream_ptr()), "mavlm_attention_colsum_batch_varlen")
        torch.cuda.synchronize()
        out, at = [], 0
        for s, n, (_, planes) in zip(keys, per, plans):
            assert bool((buf[at + planes * H * s:at + n] == SENTINEL).all()), "written behind a video's planes"
            out.append(buf[at:at + H * s].view(H, s).clone())
            at += n
        assert _intact(buf, at)
        return out
    got, ln = _counted(launch)
    assert ln == {"attention_colsum": 1, "misc": 1}, ln
    assert all(torch.equal(a, b) for a, b in zip(launch(), got))
    assert all(torch.equal(a, b) for a, b in zip(ops.attention_colsum_batch_varlen(q, k, lse, H, keys, scale=scale), got))
    for b in range(nb):
        qb, lb = q[b * R:(b + 1) * R], lse[b * H:(b + 1) * H]
        _gate(f"colsum varlen R{R} S{keys[b]} H{H} video {b} (G {plans[b][0]}, {plans[b][1]} planes) {mode} {kind}", got[b],
              prob_mass_eval(qb, ks[b], lb, H, 128, c), prob_mass_eval(qb, ks[b], lb, H, 128, c, torch.float32), 32)


# --------------------------------------------------------------------------------------------------------- fused frame scores
def _cut_blocks(R, S, H, waves):
    """query blocks (of 32 x waves rows) that hold a cut unit of the forward's plan under the hooks in force"""
    lib = capi.lib()
    nqb = -(-R // (32 * waves))
    cut, b = set(), 0
    while True:
        u = lib.mavlm_attention_plan_unit(R, S, H, 0, 0, b)
        if u < 0:
            return sorted(cut)
        cut.add(u % nqb)
        b += 1


def _frame_operands(P, F, mode, kind):
    """Q, K, V of one frame shape, shared by the four forms; planted rows at a tile's edges, the last row and the first and last
    row of every block that holds a cut unit under either stream-K form (the caller sets the hooks of each form afterwards)"""
    lib = capi.lib()
    R, H, S = T.FRAMES_R, T.FRAMES_H, P * F
    q, k, v = _randn((R, H * 128), 4700 + P, mode), _randn((S, H * 128), 4800 + P, mode), _randn((S, H * 128), 4900 + P, mode)
    if kind == "planted":
        rows = _tile_rows(R, 64)
        capi.check(lib.mavlm_set_attention_streamk_min_tiles(1), "min tiles")
        for waves in (4, 8):
            capi.check(lib.mavlm_set_attention_streamk_waves(waves), "waves")
            for b in _cut_blocks(R, S, H, waves):
                rows |= {b * 32 * waves, min(R, (b + 1) * 32 * waves) - 1}
        _plant(q, k, rows)
    return q, k, v


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P,F", T.FRAMES_PF, ids=lambda v: str(v))
def test_fused_frame_scores(P, F, mode, kind):
    """attn_fwd3_kernel<T, NW, FR = 1 / 3> + attn_combine_sk_kernel + frame_finish_kernel through `mavlm_attention_frames`: the
    plain grid, the stream-K schedule on 4- and 8-wave workgroups, the 8-wave form with its entries in LDS and through the
    scratch.  Scores per frame against float64 of the contract with the lse2 the SAME launch returned."""
    lib = capi.lib()
    R, H, S = T.FRAMES_R, T.FRAMES_H, P * F
    q, k, v = _frame_operands(P, F, mode, kind)
    scale = _scale(128)
    c = attn_c32(scale)
    info = (ctypes.c_int32 * 4)()
    scores_of = {}
    for name, min_tiles, waves, lds, want in T.FRAMES_FORMS:
        capi.check(lib.mavlm_set_attention_streamk_min_tiles(min_tiles), "min tiles")
        capi.check(lib.mavlm_set_attention_streamk_waves(waves), "waves")
        capi.check(lib.mavlm_set_frame_entries_lds(lds), "hook")
        capi.check(lib.mavlm_attention_plan(R, S, H, info), "plan")
        assert list(info) == want, (name, list(info))
        nws = int(lib.mavlm_attention_frames_ws_floats(R, S, H, P))
        assert nws > 0

        def launch():
            out = torch.empty((R, H * 128), device="cuda", dtype=q.dtype)
            lse = torch.empty((H, R), device="cuda", dtype=torch.float32)
            ws = torch.empty((nws,), device="cuda", dtype=torch.float32)
            sc = _guarded(F)
            capi.check(lib.mavlm_attention_frames(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                                  out.data_ptr(), out.stride(0), lse.data_ptr(), R, S, H, scale, P, ws.data_ptr(), nws,
                                                  sc.data_ptr(), ops.dtype_code(q.dtype), ops.stream_ptr()), "mavlm_attention_frames")
            torch.cuda.synchronize()
            assert _intact(sc, F)
            return out, lse, sc[:F].clone()
        (out, lse, scores), ln = _counted(launch)
        assert ln.get("attention_fwd_frames") == 1 and "attention_colsum" not in ln and "attention_fwd" not in ln, (name, ln)
        assert (ln.get("attention_merge", 0) == 1) == (want[1] > 0) and ln.get("misc") == 1, (name, ln)     # combine; frame_finish
        again = launch()
        assert torch.equal(again[0], out) and torch.equal(again[1], lse) and torch.equal(again[2], scores)
        per_frame = lambda col: col.view(H, F, P).sum(dim=(0, 2)) / P
        _gate(f"frames {name} R{R} P{P}xF{F} {mode} {kind}", scores, per_frame(prob_mass_eval(q, k, lse, H, 128, c)),
              per_frame(prob_mass_eval(q, k, lse, H, 128, c, torch.float32)), 1)
        scores_of[name] = scores
    assert torch.equal(scores_of["sk8-lds"], scores_of["sk8-scratch"])


# -------------------------------------------------------------------------------------------------------------- attention maps
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hd,R,S,H,qg,kg", T.MAP_CASES, ids=lambda v: str(v))
def test_attention_maps(hd, R, S, H, qg, kg, mode, kind):
    """attn_group_mass_rows_kernel<T, 128 / 448> + attn_group_mass_reduce_kernel: cells per key group, a ragged last group on
    both axes, key-group ranges (grid y) that end inside a 32-key tile"""
    lib = capi.lib()
    q, k = _randn((R, H * hd), 5000 + hd, mode), _randn((S, H * hd), 5100 + hd, mode)
    if kind == "planted":
        # (a map row of ONE query row scaled by 8 holds cells of 2^-130 and less, which fp32 flushes to zero - there is no fp32
        #  floor for them: with q_group 1 every planted row is scaled by 2, cells of 2^-30, well inside fp32)
        _plant(q, k, _tile_rows(R, 32) | {127, 128}, 8.0 if qg > 1 else 2.0)
    scale = _scale(hd)
    c = attn_c32(scale)
    lse = _lse_input(q, k, H, hd, c)
    nq, nk = -(-R // qg), -(-S // kg)
    n = int(lib.mavlm_attention_group_mass_floats(R, S, H, qg, kg))
    assert n == H * nq * nk + H * nk * R

    def launch():
        buf = _guarded(n)
        capi.check(lib.mavlm_attention_group_mass(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), lse.data_ptr(), buf.data_ptr(), n,
                                                  R, S, H, hd, scale, qg, kg, ops.dtype_code(q.dtype), ops.stream_ptr()),
                   "mavlm_attention_group_mass")
        torch.cuda.synchronize()
        assert _intact(buf, n)
        return buf[:H * nq * nk].view(H, nq, nk).clone()
    got, ln = _counted(launch)
    assert ln == {"attention_colsum": 2}, ln                     # the rows kernel and the reduce
    assert torch.equal(launch(), got)
    assert torch.equal(ops.attention_group_mass(q, k, lse, H, qg, kg, head_dim=hd, scale=scale), got)
    exp = None
    if _single_exponent(hd, kind, qg):                           # additions: the quads of a key group, the rows of a query group
        exp = prob_mass_eval(q, k, lse, H, hd, c, torch.float64, qg, kg, rounding="expected", adds=kg // 4 + qg // 64 + 8)
    _gate(f"maps hd{hd} R{R} S{S} H{H} groups ({qg}, {kg}) {mode} {kind}", got, prob_mass_eval(q, k, lse, H, hd, c, torch.float64, qg, kg),
          prob_mass_eval(q, k, lse, H, hd, c, torch.float32, qg, kg), 1, exp)
