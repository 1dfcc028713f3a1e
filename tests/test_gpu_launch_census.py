"""-m gpu: the pinned launch census of the host layer (csrc/mavlm_{context,step,emit,ops}.hip).  Every scenario runs once with
the library's profile on (`mavlm_prof_enable` / `mavlm_prof_read`) and the launches, algorithmic flops and bytes per kernel kind
(`capi.KERNEL_KINDS`) must EQUAL `tests/launch_census.json` - integers, compared exactly.  The bit-for-bit tests of the other
modules do not see a dropped split-K workspace or another route to the same values; a count does.

The fixture is never recorded from the code under test: it comes from the commit BEFORE the change (`record_census`, see
tests/README.md).  Every scenario builds its own model, so no cached first-step Q or engine of another test moves a count.

Default shape (tests/test_gpu_ragged_batch.py): D = 256, 2 heads of 128, M = 2, P = 196, chunks of 4 frames, FIFO of 2, depth 2."""
import ctypes
import json
import os

import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from memory_augmented_vlm_amd.model import llava_arch as arch
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector, _Engine
from oracle import memory_path as O
from gpu_util import to_dev
from test_gpu_batch import _host, _prompts

pytestmark = pytest.mark.gpu
P, CHUNK, CAP, FINE = 196, 4, 2, 3
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_census.json")


class _Case:
    """a fresh model (so fresh engines: nothing cached) at one width, its prompts and videos"""

    def __init__(self, mode="bf16", hidden=256, heads=2):
        cfg = O.PathConfig(hidden=hidden, heads=heads, mem_tokens=2, depth=2, cache_cap=CAP, chunk=CHUNK, fine_frames=FINE)
        self.model = _host(cfg, O.make_weights(cfg, seed=71), mode, cap=CAP, vocab=16)
        self.rm = self.model.recurrent_memory_transformer
        self.mp, self.fp = _prompts(hidden, mode)
        self.nl = self.model.image_newline.detach()
        self.mode, self.D = mode, hidden
        self.dev, self.dt = self.mp.device, self.mp.dtype

    def video(self, frames, seed):
        return to_dev(O.rounder(self.mode)(O.hash_normal_like((frames, P, self.D), seed)), self.mode), torch.arange(frames)

    def single(self, vid, idx, layout):
        arch.video_memory_tokens(self.model, vid, idx, self.mp, self.fp, self.nl, True, chunk=CHUNK, fine_frames=FINE, layout=layout)

    def batched(self, bp, vids, idxs, layout, **kw):
        return arch.video_memory_tokens_batched(self.model, bp, vids, idxs, self.mp, self.fp, self.nl, chunk=CHUNK,
                                                fine_frames=FINE, layout=layout, **kw)

    def clips(self, bp, frames, seed):
        vids, idxs = zip(*[self.video(f, seed + i) for i, f in enumerate(frames)])
        arch.video_memory_tokens_clips(self.model, bp, list(vids), list(idxs), self.mp, self.fp, self.nl, chunk=CHUNK,
                                       fine_frames=FINE, layout="frame")


def _census(fn):
    lib = capi.lib()
    nk = len(capi.KERNEL_KINDS)
    ms, fl, by = (ctypes.c_double * nk)(), (ctypes.c_double * nk)(), (ctypes.c_double * nk)()
    ln = (ctypes.c_int64 * nk)()
    torch.cuda.synchronize()
    lib.mavlm_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        capi.check(lib.mavlm_prof_read(ms, ln, fl, by, nk), "mavlm_prof_read")
    finally:
        lib.mavlm_prof_enable(0)
    assert all(fl[k] == int(fl[k]) and by[k] == int(by[k]) for k in range(nk))
    return {kind: [int(ln[k]), int(fl[k]), int(by[k])] for k, kind in enumerate(capi.KERNEL_KINDS) if ln[k]}


def _steps(ctx, segs, scores_f32=True):
    lib = capi.lib()
    capi.check(lib.mavlm_reset(ctx), "mavlm_reset")
    scores = torch.empty(CHUNK, device="cuda", dtype=torch.float32)
    for s in segs:
        capi.check(lib.mavlm_step(ctx, s.data_ptr(), s.shape[0], scores.data_ptr(), 1 if scores_f32 else 0, ops.stream_ptr()), "mavlm_step")


def _a_frame_score_modes():
    """(a) one video, 5 steps (the FIFO of 2 wraps), fp32 frame scores, under every frame-score mode"""
    c = _Case()
    vid, _ = c.video(5 * CHUNK, 100)
    segs = [vid[i * CHUNK:(i + 1) * CHUNK] for i in range(5)]
    eng = c.rm.engine(c.dev, c.dt, CHUNK)
    out = {}
    try:
        for mode in (0, 1, 2):
            capi.check(capi.lib().mavlm_set_frame_score_mode(mode), "mavlm_set_frame_score_mode")
            out[f"mode{mode}"] = _census(lambda: _steps(eng.ctx, segs))
    finally:
        capi.lib().mavlm_set_frame_score_mode(1)
    return out


def _b_layouts():
    """(b) one video emitted in each layout, with fine frames (the scratch + spread_rows route and the row-map route)"""
    c = _Case()
    vid, idx = c.video(3 * CHUNK, 110)
    return {layout: _census(lambda: c.single(vid, idx, layout)) for layout in ("one_token", "no_token", "frame", "grid")}


def _c_prefetch():
    """(c) mavlm_project_chunk / _ahead feeding steps: two hits and one discarded projection"""
    c = _Case()
    lib = capi.lib()
    vid, _ = c.video(5 * CHUNK, 120)
    seg = [vid[i * CHUNK:(i + 1) * CHUNK] for i in range(5)]
    eng = c.rm.engine(c.dev, c.dt, CHUNK)
    side = torch.cuda.Stream()
    scores = torch.empty(CHUNK, device="cuda", dtype=torch.float32)

    def step(x):
        capi.check(lib.mavlm_step(eng.ctx, x.data_ptr(), CHUNK, scores.data_ptr(), 1, ops.stream_ptr()), "mavlm_step")

    def run():
        capi.check(lib.mavlm_reset(eng.ctx), "mavlm_reset")
        capi.check(lib.mavlm_project_chunk(eng.ctx, seg[0].data_ptr(), CHUNK, ops.stream_ptr()), "mavlm_project_chunk")
        step(seg[0])                                                 # hit
        side.wait_stream(torch.cuda.current_stream())
        capi.check(lib.mavlm_project_chunk_ahead(eng.ctx, seg[2].data_ptr(), CHUNK, side.cuda_stream), "mavlm_project_chunk_ahead")
        step(seg[1])                                                 # inline projection, beside the one made ahead
        step(seg[2])                                                 # hit
        capi.check(lib.mavlm_project_chunk(eng.ctx, seg[3].data_ptr(), CHUNK, ops.stream_ptr()), "mavlm_project_chunk")
        step(seg[4])                                                 # another chunk: the projection is discarded
        torch.cuda.current_stream().wait_stream(side)

    hits = lib.mavlm_prefetch_hits(eng.ctx)
    out = _census(run)
    out["prefetch_hits"] = lib.mavlm_prefetch_hits(eng.ctx) - hits
    return {"run": out}


def _d_maps():
    """(d) attention maps bound, two steps"""
    c = _Case()
    vid, _ = c.video(2 * CHUNK, 130)
    c.rm.record_attention_maps = True

    def run():
        c.rm.memory_cache = []
        c.rm(vid[:CHUNK])
        c.rm(vid[CHUNK:])

    return {"run": _census(run)}


def _e_row_shard():
    """(e) a row shard: memory token 1 of 2"""
    c = _Case()
    vid, _ = c.video(2 * CHUNK, 140)
    eng = _Engine(c.rm, torch.device("cuda", torch.cuda.current_device()), c.dt, CHUNK, shard=(1, 1))
    eng.pack(c.rm)
    return {"run": _census(lambda: _steps(eng.ctx, [vid[:CHUNK], vid[CHUNK:]]))}


def _f_row_batch(mode="bf16"):
    """(f) row batch of 2: steps, mavlm_fuse_emit_layout_batch, and _batch_to with scattered destinations"""
    c = _Case(mode)
    T = 3 * CHUNK
    vids, idx = [c.video(T, 150 + b)[0] for b in range(2)], torch.arange(T)
    bp = BatchedProjector(c.rm, 2)
    rows = arch.video_token_rows(T, 2, P, True, CHUNK, FINE, CAP, c.mp.shape[0], c.fp.shape[0], "grid")
    out = torch.empty((3 * rows + 40, c.D), device="cuda", dtype=c.dt)
    return {"batch": _census(lambda: c.batched(bp, vids, idx, "frame")),
            "batch_to": _census(lambda: c.batched(bp, vids, idx, "grid", out=out, dst_rows=[2 * rows + 24, 8]))}


def _g_ragged():
    """(g) engine of 4 stepping prefixes 4, 3, 2, 1, then mavlm_fuse_emit_layout_ragged_to in `grid`"""
    c = _Case()
    vids, idxs = zip(*[c.video(n * CHUNK, 160 + n) for n in (4, 3, 2, 1)])
    bp = BatchedProjector(c.rm, 4)
    return {"run": _census(lambda: c.batched(bp, list(vids), list(idxs), "grid", ragged=True))}


def _h_clips():
    """(h) mavlm_step_batch_frames with unequal frame counts and scores, then mavlm_fuse_emit_layout_frames_to"""
    c = _Case()
    bp = BatchedProjector(c.rm, 3)
    return {"run": _census(lambda: c.clips(bp, (3, 2, 1), 170))}


def _i_hidden_896():
    """(i) hidden 896: 7 heads of 128 (narrow-width row-mapped emit, batch of 2); 2 heads of 448 (single video, and a batch of 2 with
    unequal frame counts: the per-video wide-head loops)"""
    out = {}
    c = _Case(hidden=896, heads=7)
    T = 2 * CHUNK
    vids, idx = [c.video(T, 180 + b)[0] for b in range(2)], torch.arange(T)
    bp = BatchedProjector(c.rm, 2)
    out["heads7_batch"] = _census(lambda: c.batched(bp, vids, idx, "grid"))
    del c, bp
    c = _Case(hidden=896, heads=2)
    vid, idx = c.video(2 * CHUNK, 190)
    out["heads2_single"] = _census(lambda: c.single(vid, idx, "frame"))
    bp = BatchedProjector(c.rm, 2)
    segs = [c.video(f, 195 + f)[0] for f in (3, 2)]

    def frames_step():            # (the clip emit needs a hidden size that is a multiple of 256: the step alone)
        bp.reset()
        bp.step_frames(segs)

    out["heads2_step_frames"] = _census(frames_step)
    return out


SCENARIOS = {"a_frame_score_modes": _a_frame_score_modes, "b_layouts": _b_layouts, "c_prefetch": _c_prefetch, "d_maps": _d_maps,
             "e_row_shard": _e_row_shard, "f_row_batch": _f_row_batch, "g_ragged": _g_ragged, "h_clips": _h_clips,
             "i_hidden_896": _i_hidden_896, "j_row_batch_fp16": lambda: _f_row_batch("fp16")}


def record_census(path=FIXTURE):
    """Writes the fixture.  Run it on a checkout of the commit BEFORE a change of the launch sequence (tests/README.md)."""
    with torch.no_grad():
        census = {name: fn() for name, fn in SCENARIOS.items()}
    with open(path, "w") as fh:
        json.dump(census, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return census


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_launch_census_equals_the_recorded_one(name):
    with open(FIXTURE) as fh:
        want = json.load(fh)[name]
    with torch.no_grad():
        got = SCENARIOS[name]()
    for part in sorted(set(want) | set(got)):
        print(name, part, json.dumps(got.get(part), sort_keys=True))
        assert got.get(part) == want.get(part), f"{name} / {part}: launches, flops or bytes of a kernel kind differ from the recorded census"
