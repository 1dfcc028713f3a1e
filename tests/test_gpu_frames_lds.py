"""-m gpu: the frame-score forward that keeps the (a, m) entries of whole units in LDS (attention3.hip FR = 3,
`mavlm_set_frame_entries_lds`, default on) against the form that sends every entry through the workspace (FR = 1, hook off).

Both forms compute the same values and add them in the same order, so everything is compared bit for bit: the context, lse2 and
the frame scores of the two forms, and context / lse2 against the forward without frame scores on the same schedule.  (The
never-split grid of `ops.attention(plain=True)` is another schedule for the cut units - it has no stream-K merge - and is gated
against float64 like every forward.)  The scores are gated against float64 column sums (torch, on the GPU) with the tolerance of
the existing frame-score tests.  Which kernel ran is read from the scratch: it is filled with a sentinel before the launch, and
with the LDS form the entries of every whole unit still hold it afterwards, while without it they have all been overwritten."""
import ctypes
import functools
import math

import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
from oracle import memory_path as O
from gpu_util import attention_gate, rel_l2_t, to_dev
from test_gpu_path import make_projector

pytestmark = pytest.mark.gpu
TOL = 1e-3                       # the gate of the existing frame-score tests (test_gpu_ops.py, test_gpu_batch.py)
SENTINEL = 1.0e30
H, R = 8, 8348                   # 33 query blocks of 256 (the last ragged) x 8 heads = 264 units: one whole round + 8 cut units


@pytest.fixture(autouse=True)
def _inference_path(request):
    lib = capi.lib()
    request.addfinalizer(lambda: (lib.mavlm_set_frame_entries_lds(1), lib.mavlm_set_attention_streamk_min_tiles(64)))
    with torch.no_grad():
        yield


def _plan(R_, S, H_):
    """(waves, whole rounds, levels, set of cut units) of the forward's schedule; unit = head * blocks + block"""
    lib = capi.lib()
    info = (capi.i32 * 4)()
    capi.check(lib.mavlm_attention_plan(R_, S, H_, info), "plan")
    waves, wgs, nlev = info[0], info[1], info[2]
    cut = set()
    for lv in range(nlev):
        b = 0
        while True:
            u = lib.mavlm_attention_plan_unit(R_, S, H_, lv, 0, b)
            if u < 0:
                break
            cut.add(u)
            b += 1
    units = -(-R_ // (32 * waves)) * H_
    return waves, (units - len(cut)) // max(wgs, 1), nlev, cut


def _frames_launch(q, k, v, P, ws):
    """`mavlm_attention_frames` on a caller-filled workspace: (ctx, lse2, scores)"""
    lib = capi.lib()
    R_, S = q.shape[0], k.shape[0]
    out = torch.empty((R_, H * 128), device=q.device, dtype=q.dtype)
    lse = torch.empty((H, R_), device=q.device, dtype=torch.float32)
    scores = torch.empty((S // P,), device=q.device, dtype=torch.float32)
    capi.check(lib.mavlm_attention_frames(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                          out.data_ptr(), out.stride(0), lse.data_ptr(), R_, S, H, 1.0 / math.sqrt(128.0), P,
                                          ws.data_ptr(), ws.numel(), scores.data_ptr(), ops.dtype_code(q.dtype), ops.stream_ptr()),
               "mavlm_attention_frames")
    return out, lse, scores


@functools.lru_cache(maxsize=None)
def _case(mode, FN, P):
    """operands (device, 16-bit) and the float64 reference of one shape, computed once: ctx, lse2 (log2 domain), frame scores"""
    S = FN * P
    r = O.rounder(mode)
    q = r(O.hash_normal_like((R, H * 128), 171))
    k = r(O.hash_normal_like((S, H * 128), 172))
    v = r(O.hash_normal_like((S, H * 128), 173))
    _, _, _, cut = _plan(R, S, H)
    nqb = -(-R // 256)
    cut_blocks = sorted({u % nqb for u in cut})
    whole_blocks = [b for b in range(nqb) if all(h * nqb + b not in cut for h in range(H))]
    # rows whose maximum jumps by far more than 2^8 (log2 domain: 6 |q_h|^2 / sqrt(128) log2 e ~ 100) late in the key sequence:
    # in the middle of a frame, in the first tile behind a frame boundary, and inside a cut unit (its last piece)
    row_mid, row_edge, row_cut = whole_blocks[1] * 256 + 5, whole_blocks[2] * 256 + 40, cut_blocks[0] * 256 + 37
    assert row_cut < R
    s_mid = (FN - 2) * P + P // 2
    s_edge = -(-((FN // 2) * P) // 64) * 64 + 3
    s_cut = (FN - 1) * P + 5
    for row, s0 in ((row_mid, s_mid), (row_edge, s_edge), (row_cut, s_cut)):
        k[s0:s0 + 8] = r(q[row][None, :] * 6.0)
    dq, dk, dv = to_dev(q, mode), to_dev(k, mode), to_dev(v, mode)
    scale = 1.0 / math.sqrt(128.0)
    col = torch.zeros((S,), device="cuda", dtype=torch.float64)
    ctx = torch.empty((R, H * 128), device="cuda", dtype=torch.float64)
    lse2 = torch.empty((H, R), device="cuda", dtype=torch.float64)
    for h in range(H):
        sl = slice(h * 128, (h + 1) * 128)
        kh, vh = dk[:, sl].double(), dv[:, sl].double()
        for r0 in range(0, R, 2048):
            s = (dq[r0:r0 + 2048, sl].double() @ kh.T) * scale
            l = torch.logsumexp(s, dim=1, keepdim=True)
            p = torch.exp(s - l)
            col += p.sum(0)
            ctx[r0:r0 + 2048, sl] = p @ vh
            lse2[h, r0:r0 + 2048] = l[:, 0] * 1.4426950408889634
    return dq, dk, dv, ctx, lse2, col.view(FN, P).mean(1)


def _whole_unit_entries(ws, S, P, cut):
    """the (a, m) scratch entries of the rows of every whole unit: [n, FN, 2]"""
    FN = S // P
    FNE = FN + 31
    scr = ws[:H * R * FNE * 2].view(H, R, FNE, 2)
    nqb = -(-R // 256)
    keep = [scr[u // nqb, (u % nqb) * 256:min(R, (u % nqb + 1) * 256), :FN] for u in range(H * nqb) if u not in cut]
    return torch.cat(keep, 0)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("FN,P,lds", [(21, 196, True),     # 65 key tiles, the last ragged
                                      (32, 196, True),     # the most frames the LDS form takes
                                      (33, 196, False),    # one more: falls back to the scratch form
                                      (32, 64, True)])     # the smallest frame: a boundary at the end of every tile
def test_frame_entries_in_lds_equal_the_scratch_form(mode, FN, P, lds):
    lib = capi.lib()
    S = FN * P
    if -(-S // 64) < 64:                                   # (few key tiles: the stream-K plan from 2 tiles on, as the existing tests)
        capi.check(lib.mavlm_set_attention_streamk_min_tiles(2), "min tiles")
    waves, rounds, nlev, cut = _plan(R, S, H)
    assert waves == 8, "the shape must take the 8-wave stream-K plan"
    assert rounds >= 1, "at least one whole round"
    assert nlev >= 1 and len(cut) >= 1, "at least one cut level"
    dq, dk, dv, ref_ctx, ref_lse2, ref_scores = _case(mode, FN, P)
    nws = int(lib.mavlm_attention_frames_ws_floats(R, S, H, P))
    assert nws > 0
    res = {}
    for on in (1, 0):
        capi.check(lib.mavlm_set_frame_entries_lds(on), "hook")
        ws = torch.full((nws,), SENTINEL, device="cuda", dtype=torch.float32)
        res[on] = _frames_launch(dq, dk, dv, P, ws)
        ent = _whole_unit_entries(ws, S, P, cut)
        if on and lds:                                     # whole units never touched the scratch ...
            assert bool((ent == SENTINEL).all()), "a whole unit wrote frame entries to the scratch"
        else:                                              # ... and the scratch form overwrote every entry of theirs
            assert bool((ent != SENTINEL).all())
    for a, b in zip(res[1], res[0]):                       # ctx, lse2, scores: hook on == hook off
        assert torch.equal(a, b)
    plain, lse_p = ops.attention(dq, dk, dv, H, want_lse=True)        # the forward without frame scores, same schedule
    if not (torch.equal(res[1][0], plain) and torch.equal(res[1][1], lse_p)):
        # which side is off, where, and does it repeat: each side's distance from float64 on the rows that differ, a second
        # launch of each, printed before the assertion reports the mismatch
        nqb = -(-R // 256)
        d = (res[1][0] != plain).view(R, H, 128).any(2) | (res[1][1] != lse_p).t()
        pairs = d.nonzero().tolist()
        units = sorted({h * nqb + r_ // 256 for r_, h in pairs})
        m = d[:, :, None].expand(R, H, 128).reshape(R, H * 128)
        e_f = float((res[1][0].double() - ref_ctx)[m].norm())
        e_p = float((plain.double() - ref_ctx)[m].norm())
        again, lse_a = ops.attention(dq, dk, dv, H, want_lse=True)
        ws = torch.full((nws,), SENTINEL, device="cuda", dtype=torch.float32)
        fr_again = _frames_launch(dq, dk, dv, P, ws)
        print(f"[{mode} FN={FN} P={P}] frames != plain in {len(pairs)} (row, head) pairs; units {units[:16]} (cut: "
              f"{[u in cut for u in units[:16]]}); rows {sorted({r_ for r_, _ in pairs})[:16]}; error against float64 on those "
              f"rows: frames {e_f:.3e}, plain {e_p:.3e}; second plain launch == first: "
              f"{torch.equal(again, plain) and torch.equal(lse_a, lse_p)}, == frames: {torch.equal(again, res[1][0])}; second "
              f"frames launch == first: {torch.equal(fr_again[0], res[1][0])}, == plain: {torch.equal(fr_again[0], plain)}")
    assert torch.equal(res[1][0], plain) and torch.equal(res[1][1], lse_p)
    never_split, lse_n = ops.attention(dq, dk, dv, H, want_lse=True, plain=True)
    for name, (c_, l_) in (("frames", res[1][:2]), ("never-split", (never_split, lse_n))):
        g, lerr, ok = attention_gate(c_, l_, ref_ctx, ref_lse2, H, mode)
        print(f"[{mode} FN={FN} P={P}] {name}: {g}; lse2 {lerr:.2e}")
        assert ok
    scores = res[1][2]
    err = rel_l2_t(scores, ref_scores)
    print(f"[{mode} FN={FN} P={P}] frame scores vs float64 column sums: {err:.2e}")
    assert err < TOL and abs(float(scores.sum()) * P - H * R) < 1e-3 * H * R
    capi.check(lib.mavlm_set_frame_entries_lds(1), "hook")
    ws = torch.full((nws,), -SENTINEL, device="cuda", dtype=torch.float32)     # another sentinel: the result does not move
    assert torch.equal(_frames_launch(dq, dk, dv, P, ws)[2], scores)


def test_row_batch_step_with_frame_entries_in_lds():
    """A row batch of 2 through `mavlm_step_batch` at hidden 1024 with 43 memory tokens and one 21-frame chunk (16 (video, head)
    pairs x 33 query blocks: two whole rounds + 16 cut units on the 8-wave plan): memory and frame scores with the hook on equal
    the hook off bit for bit."""
    lib = capi.lib()
    cfg = O.PathConfig(hidden=1024, heads=8, mem_tokens=43, depth=2)
    Rr, S = 43 * 196, 21 * 196
    waves, rounds, nlev, cut = _plan(Rr, S, 16)
    assert waves == 8 and rounds >= 1 and nlev >= 1 and cut
    assert lib.mavlm_attention_frames_ws_floats(Rr, S, 16, 196) > 0
    rm = make_projector(cfg, O.make_weights(cfg, seed=181)).to("cuda").to(torch.bfloat16)
    segs = [to_dev(O.bf16_round(O.hash_normal_like((21, 196, 1024), 1810 + b))) for b in range(2)]
    bp = BatchedProjector(rm, 2)
    bp.reset()
    bp.step(segs)                                          # (engine, packing, the one-time memset: outside the counted step)
    got = {}
    nk = len(capi.KERNEL_KINDS)
    for on in (1, 0):
        capi.check(lib.mavlm_set_frame_entries_lds(on), "hook")
        bp.reset()
        torch.cuda.synchronize()
        lib.mavlm_prof_enable(1)                           # launch counters: which forward the last layer of the step ran
        try:
            scores = bp.step(segs).clone()
            torch.cuda.synchronize()
            ms, fl, by = (ctypes.c_double * nk)(), (ctypes.c_double * nk)(), (ctypes.c_double * nk)()
            ln = (ctypes.c_int64 * nk)()
            capi.check(lib.mavlm_prof_read(ms, ln, fl, by, nk), "mavlm_prof_read")
        finally:
            lib.mavlm_prof_enable(0)
        # the fused frame-score forward ran (one launch for the last of the two layers), not the column-sum pass
        assert ln[capi.KERNEL_KINDS.index("attention_fwd_frames")] == 1 and ln[capi.KERNEL_KINDS.index("attention_colsum")] == 0
        assert ln[capi.KERNEL_KINDS.index("attention_fwd")] == 1
        got[on] = (scores, [bp.memory_cache(b)[-1].clone() for b in range(2)])
    assert torch.equal(got[1][0], got[0][0])
    assert all(torch.equal(u, v_) for u, v_ in zip(got[1][1], got[0][1]))
    assert bool(torch.isfinite(got[1][0].float()).all()) and abs(float(got[1][0].float().sum()) * 196 / (8 * Rr * 2) - 1.0) < 2e-2
