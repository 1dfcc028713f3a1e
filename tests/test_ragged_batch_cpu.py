"""CPU (-m "not gpu") tests of ragged row batches: the planner, the binding of the new exports and the refusals that need no
device.  (The refusal of a prefix that grows needs a step to have run first: tests/test_gpu_ragged_batch.py.)"""
import ctypes
import os
import re

import pytest
import torch

import memory_augmented_vlm_amd as pkg
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd.model import llava_arch as arch
from conftest import ROOT


@pytest.fixture(scope="module")
def built_lib():
    return pkg.build_library()


def lengths(*chunks):
    return [32 * c for c in chunks]


def test_planner_orders_longest_first_and_keeps_input_order_among_equals():
    # chunk counts 2, 3, 2, 4 + one video of 20 frames (not a multiple of the chunk)
    ragged, batches, singles = arch.plan_ragged_batches([64, 96, 64, 128, 20])
    assert ragged == [(4, [3, 1, 0, 2])] and batches == [] and singles == [4]
    # equal counts: input order
    assert arch.plan_ragged_batches(lengths(3, 3, 3)) == ([(4, [0, 1, 2])], [], [])


def test_planner_half_rule_opens_a_new_group():
    # 8, 6, 4, 4 stay with the 8 (4 >= 8 / 2); 3 does not (2 * 3 < 8) and opens the next group, whose bound is 3 / 2
    ragged, batches, singles = arch.plan_ragged_batches(lengths(2, 2, 3, 3, 4, 4, 6, 8))
    assert ragged == [(4, [2, 3, 0, 1]), (4, [7, 6, 4, 5])] and batches == [] and singles == []
    # a lopsided pair never shares a batch: two singles
    assert arch.plan_ragged_batches(lengths(2, 16)) == ([], [], [0, 1])
    # ... and a group of one goes where it goes today: the three 2-chunk videos form a group, the 16-chunk one is a single
    assert arch.plan_ragged_batches(lengths(2, 16, 2, 2)) == ([(4, [0, 2, 3])], [], [1])


def test_planner_group_never_exceeds_eight():
    ragged, batches, singles = arch.plan_ragged_batches(lengths(*([4] * 11)))
    assert ragged == [(8, list(range(8))), (4, [8, 9, 10])] and batches == [] and singles == []
    ragged, _, singles = arch.plan_ragged_batches(lengths(*([4] * 9)))
    assert ragged == [(8, list(range(8)))] and singles == [8]


@pytest.mark.parametrize("k, size", [(2, 2), (3, 4), (4, 4), (5, 8), (6, 8), (7, 8), (8, 8)])
def test_planner_one_engine_per_group(k, size):
    ragged, batches, singles = arch.plan_ragged_batches(lengths(*range(k + 7, 7, -1)))      # all within the half rule
    assert ragged == [(size, list(range(k)))] and batches == [] and singles == []


def test_planner_ineligible_lengths_fall_back_to_the_equal_length_plan():
    lens = [20, 20, 33, 33, 33, 7]
    keys = [("bf16", "cuda:0")] * 6
    ragged, batches, singles = arch.plan_ragged_batches(lens, 32, keys)
    b0, s0 = arch.plan_row_batches([(t, k) for t, k in zip(lens, keys)])
    assert ragged == [] and (batches, singles) == (b0, s0) == ([[0, 1], [2, 3]], [4, 5])
    # mixed: the eligible ones are planned ragged, the rest exactly as before, positions in input order
    ragged, batches, singles = arch.plan_ragged_batches([20, 64, 20, 96, 40], 32)
    assert ragged == [(2, [3, 1])] and batches == [[0, 2]] and singles == [4]
    # another dtype / device never shares a batch
    ragged, batches, singles = arch.plan_ragged_batches([64, 96], 32, ["a", "b"])
    assert ragged == [] and batches == [] and singles == [0, 1]
    # another chunk size
    assert arch.plan_ragged_batches([8, 4, 6], 4) == ([(2, [0, 1])], [], [2])


def test_planner_empty_and_single():
    assert arch.plan_ragged_batches([]) == ([], [], [])
    assert arch.plan_ragged_batches([64]) == ([], [], [0])
    assert arch.plan_ragged_batches([5]) == ([], [], [0])
    with pytest.raises(ValueError):
        arch.plan_ragged_batches([64, 64], sizes=(1,))
    with pytest.raises(ValueError):
        arch.plan_ragged_batches([64, 64], keys=[None])


def test_new_exports_are_declared_and_bound(built_lib):
    hdr = open(os.path.join(ROOT, "include", "mavlm.h")).read()
    l = ctypes.CDLL(built_lib)
    for name in ("mavlm_step_batch_active", "mavlm_video_steps", "mavlm_fuse_emit_layout_ragged_to"):
        assert name in capi.SIGNATURES and hasattr(l, name)
        assert re.search(r"\bint %s\(" % name, hdr)
    assert "llava_arch.py:436,534-537" in hdr and "llava_arch.py:436,545-554" in hdr
    assert capi.lib().mavlm_abi_version() == 3


def cfg(batch):
    return capi.Config(hidden=256, heads=2, patches=196, mem_tokens=2, depth=2, inter=1024, cache_cap=2, max_chunk_frames=4,
                       dtype=0, eps=1e-12, batch=batch)


def test_step_refusals_without_a_device(built_lib):
    lib = capi.lib()
    h = capi.vp()
    assert lib.mavlm_create(cfg(4), h) == 0
    segs = (capi.vp * 4)(256, 256, 256, 256)
    assert lib.mavlm_step_batch_active(h, segs, 0, 4, None, 0, None) == capi.E_ARG
    assert lib.mavlm_step_batch_active(h, segs, 5, 4, None, 0, None) == capi.E_ARG
    assert lib.mavlm_step_batch_active(h, segs, -1, 4, None, 0, None) == capi.E_ARG
    assert lib.mavlm_step_batch_active(h, None, 2, 4, None, 0, None) == capi.E_ARG
    assert lib.mavlm_step_batch_active(h, segs, 2, 4, None, 0, None) == capi.E_STATE     # nothing bound yet
    assert lib.mavlm_steps(h) == 0 and [lib.mavlm_video_steps(h, b) for b in range(4)] == [0] * 4
    assert lib.mavlm_video_steps(h, 4) == capi.E_ARG and lib.mavlm_video_steps(h, -1) == capi.E_ARG
    lib.mavlm_destroy(h)
    h1 = capi.vp()
    assert lib.mavlm_create(cfg(0), h1) == 0                                             # a single-video context
    assert lib.mavlm_step_batch_active(h1, segs, 1, 4, None, 0, None) == capi.E_STATE
    assert lib.mavlm_step_batch_active(h1, segs, 2, 4, None, 0, None) == capi.E_ARG
    assert lib.mavlm_video_steps(h1, 0) == 0
    lib.mavlm_destroy(h1)


def test_workspace_of_a_row_batch_keeps_its_regions(built_lib):
    """what the smaller video counts need lies behind the regions of the full batch: the reported offsets are those of a carve
    that knows nothing of prefixes (regions in carve order, each at the end of the one before), and the total only grows"""
    lib = capi.lib()
    for c in (cfg(4), cfg(8), capi.Config(hidden=1024, heads=8, patches=196, mem_tokens=8, depth=2, inter=4096, cache_cap=10,
                                          max_chunk_frames=32, dtype=0, eps=1e-12, batch=4)):
        off = (ctypes.c_size_t * 14)()
        assert lib.mavlm_workspace_layout(c, off, 14) == 0
        assert list(off[:10]) == sorted(off[:10]) and off[0] == 0
        assert lib.mavlm_workspace_bytes(c) > off[10] + off[11]


def test_ragged_emit_refusals_without_a_device(built_lib):
    lib = capi.lib()
    h = capi.vp()
    assert lib.mavlm_create(cfg(4), h) == 0
    rows = (ctypes.c_int64 * 4)()
    xs = (capi.vp * 4)(256, 256, 256, 256)

    def emit(n, dst, out_rows, out=4096, ctx=h, layout=capi.LAYOUT_NONE, newline=None):
        return lib.mavlm_fuse_emit_layout_ragged_to(ctx, n, xs, 512, 2, 1024, 3, 2048, 2, newline, 1, layout, out, out_rows,
                                                    (ctypes.c_int64 * len(dst))(*dst), rows, None)

    # no video has stepped: a block is [3 prompt rows ; 2 prompt rows ; 2 fine frames] = 3 + 2 + 392 rows
    need = 3 + 2 + 2 * 196
    assert emit(2, [0, need], 2 * need) == capi.E_STATE                   # destinations fine, nothing bound: state
    assert emit(2, [0, need - 1], 2 * need) == capi.E_ARG                 # overlapping
    assert emit(2, [need - 1, 0], 2 * need) == capi.E_ARG
    assert emit(2, [0, 0], 2 * need) == capi.E_ARG
    assert emit(2, [0, need + 1], 2 * need) == capi.E_ARG                 # past the end of `out`
    assert emit(2, [-1, need], 2 * need) == capi.E_ARG
    assert emit(3, [0, need, 2 * need], 3 * need - 1) == capi.E_ARG
    assert emit(0, [0], need) == capi.E_ARG and emit(5, [0] * 5, 10 * need) == capi.E_ARG
    assert emit(2, [0, need], 2 * need, out=4096 + 8) == capi.E_ARG       # 16-byte alignment
    assert emit(2, [0, need], 2 * need, layout=capi.LAYOUT_ONE) == capi.E_ARG      # a newline layout without the newline row
    assert emit(2, [0, need], 2 * need, layout=7) == capi.E_ARG
    assert list(rows) == [0] * 4
    lib.mavlm_destroy(h)
    h1 = capi.vp()
    assert lib.mavlm_create(cfg(1), h1) == 0
    assert emit(1, [0], need, ctx=h1) == capi.E_STATE                     # a single-video context
    lib.mavlm_destroy(h1)


def test_switch_is_off_by_default_and_off_means_the_equal_length_planner(monkeypatch):
    assert arch.LlavaMetaForCausalLM._ragged_row_batches is False

    class M(arch.LlavaMetaForCausalLM):
        pass

    m = M()
    m.enable_ragged_row_batches()
    assert m._ragged_row_batches is True and arch.LlavaMetaForCausalLM._ragged_row_batches is False
    m.enable_ragged_row_batches(False)
    assert m._ragged_row_batches is False

    calls = []

    class Stop(Exception):
        pass

    def spy(name, real):
        def f(*a, **k):
            calls.append(name)
            real(*a, **k)
            raise Stop
        return f

    monkeypatch.setattr(arch, "plan_row_batches", spy("equal", arch.plan_row_batches))
    monkeypatch.setattr(arch, "plan_ragged_batches", spy("ragged", arch.plan_ragged_batches))

    class Model:
        recurrent_memory_transformer = None

    vids = [(torch.zeros(64, 196, 8), None), (torch.zeros(96, 196, 8), None)]
    for kw, want in (({}, "equal"), ({"ragged": False}, "equal"), ({"ragged": True}, "ragged"),
                     ({"ragged": True, "train": True}, "equal")):
        del calls[:]
        with pytest.raises(Stop):
            arch.run_video_groups(Model(), vids, None, None, None, **kw)
        assert calls[0] == want
