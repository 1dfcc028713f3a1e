"""CPU (-m "not gpu") tests of clip row batches under autograd: the binding of the variable-length attention backward, its refusals
(every one before any launch: none needs a device), the entry-point switch and the refusals of `step_train_frames`."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import memory_augmented_vlm_amd as pkg
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _autograd as ag
from memory_augmented_vlm_amd import _ops as ops
from conftest import ROOT

NEW = "mavlm_attention_bwd_batch_varlen"


@pytest.fixture(scope="module")
def built_lib():
    return pkg.build_library()


def _S(*v):
    return (capi.i32 * len(v))(*v)


def _off(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_new_export_is_declared_and_bound(built_lib):
    hdr = open(os.path.join(ROOT, "include", "mavlm.h")).read()
    l = ctypes.CDLL(built_lib)
    assert NEW in capi.SIGNATURES and hasattr(l, NEW)
    assert re.search(r"\bint %s\(" % NEW, hdr)
    assert re.search(r"#define MAVLM_ABI_VERSION 3\b", hdr) and capi.lib().mavlm_abi_version() == 3
    # the header's parameter list and the ctypes table agree in length
    decl = re.search(r"\bint %s\(([^;]*)\);" % NEW, hdr).group(1)
    assert len(decl.split(",")) == len(capi.SIGNATURES[NEW][1]) == 28


def test_wrappers_and_autograd_form_exist():
    for f in (ops.attention_batch_varlen, ops.attention_colsum_batch_varlen, ops.attention_bwd_batch_varlen):
        assert callable(f)
    sig = inspect.signature(ag.AttentionFn.forward).parameters
    assert list(sig)[-1] == "key_counts" and sig["key_counts"].default is None and sig["nb"].default == 1
    assert inspect.signature(ag.attention_block).parameters["key_counts"].default is None


def test_varlen_backward_refusals_without_a_device(built_lib):
    lib = capi.lib()
    P, ld, R = 4096, 256, 196

    def bwd(S, off, nb, doff=None, H=None, hd=128, ldk=ld, lddk=ld, dq=P, dk=P, dv=P):
        return lib.mavlm_attention_bwd_batch_varlen(P, ld, P, ldk, P, ld, P, ld, P, ld, P, P, dq, ld, dk, lddk, dv, ld, R, _S(*S),
                                                    _off(*off), _off(*(off if doff is None else doff)), 2 * nb if H is None else H,
                                                    0.1, nb, hd, capi.BF16, None)

    S17, off17 = [64] * 17, [64 * ld * b for b in range(17)]
    assert bwd(S17, off17, 17) == capi.E_ARG                                  # more videos than the by-value arrays hold
    assert bwd([64], [0], 0) == capi.E_ARG
    assert bwd([64, 64], [0, 64 * ld], 2, H=3) == capi.E_ARG                  # H % nb
    assert bwd([64, 0], [0, 64 * ld], 2) == capi.E_ARG                        # S[b] < 1
    assert bwd([64, 64], [0, 63 * ld], 2, doff=[0, 64 * ld]) == capi.E_ARG    # video 1's keys start inside video 0's
    assert bwd([64, 64], [0, 64 * ld], 2, doff=[0, 63 * ld]) == capi.E_ARG    # video 1's key gradients start inside video 0's
    assert bwd([40, 64, 980], [0, 40 * ld, 104 * ld], 3, doff=[0, 40 * ld, 103 * ld]) == capi.E_ARG
    assert bwd([64, 64], [0, 64 * ld + 4], 2, doff=[0, 64 * ld]) == capi.E_ARG            # alignment of an offset
    assert bwd([64, 64], [0, 64 * ld], 2, doff=[0, 64 * ld + 4]) == capi.E_ARG
    assert bwd([64, 64], [0, 64 * ld], 2, doff=[0, -8]) == capi.E_ARG
    assert bwd([64, 64], [0, 64 * ld], 2, ldk=ld + 4) == capi.E_ARG           # stride alignment
    assert bwd([64, 64], [0, 64 * ld], 2, lddk=ld + 2) == capi.E_ARG
    assert bwd([64, 64], [0, 64 * ld], 2, dk=P + 4) == capi.E_ARG             # a gradient pointer that is not 8-byte aligned
    assert bwd([64, 64], [0, 64 * ld], 2, hd=448) == capi.E_SHAPE
    assert bwd([64, 64], [0, 64 * ld], 2, hd=256) == capi.E_SHAPE
    assert bwd([64, 64], [0, 64 * ld], 2, hd=0) == capi.E_SHAPE
    # a video whose keys exceed the kernel's 32-bit offsets (one tile past the end included)
    big = (1 << 31) // (2 * ld) - 64
    assert bwd([64, big], [0, 64 * ld], 2) == capi.E_ARG


def test_wrapper_refusals_on_the_host():
    """the wrappers refuse CPU tensors (no fallback) before anything else"""
    q = torch.zeros(392, 256, dtype=torch.bfloat16)
    kv = torch.zeros(104, 256, dtype=torch.bfloat16)
    with pytest.raises(capi.MavlmError):
        ops.attention_batch_varlen(q, kv, kv, 2, (40, 64))
    with pytest.raises(capi.MavlmError):
        ops.attention_bwd_batch_varlen(q, kv, kv, q, q, torch.zeros(4, 196), 2, (40, 64))


# ---- the switch and the grouping -----------------------------------------------------------------------------------------------------------
def test_training_switch_routes_clips_to_the_clip_planner(monkeypatch):
    from memory_augmented_vlm_amd.model import llava_arch as arch
    assert arch.LlavaMetaForCausalLM._clip_row_batches is False and arch.LlavaMetaForCausalLM._clip_row_batches_train is False

    class M(arch.LlavaMetaForCausalLM):
        pass

    m = M()
    m.enable_clip_row_batches()
    assert m._clip_row_batches is True and m._clip_row_batches_train is False            # the inference switch alone
    m.enable_clip_row_batches(True, training=True)
    assert m._clip_row_batches is True and m._clip_row_batches_train is True
    m.enable_clip_row_batches(False, training=True)
    assert m._clip_row_batches is False and m._clip_row_batches_train is False
    assert arch.LlavaMetaForCausalLM._clip_row_batches_train is False                    # a per-instance flag
    assert inspect.signature(arch.LlavaMetaForCausalLM.enable_clip_row_batches).parameters["training"].default is False
    assert inspect.signature(arch.run_video_groups).parameters["clips_train"].default is False
    # the clip token block has the parameters of the equal-length one (whose list tests/test_batch_train_cpu.py pins)
    assert list(inspect.signature(arch.video_memory_tokens_clips_train).parameters) == \
        list(inspect.signature(arch.video_memory_tokens_batched_train).parameters)

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
    monkeypatch.setattr(arch, "plan_clip_batches", spy("clips", arch.plan_clip_batches))

    class Model:
        recurrent_memory_transformer = None

    vids = [(torch.zeros(9, 196, 8), None), (torch.zeros(17, 196, 8), None)]
    for kw, want in (({"train": True, "clips_train": True}, "clips"), ({"train": True, "clips_train": True, "clips": True}, "clips"),
                     # without `train` the new keyword changes nothing
                     ({"clips_train": True}, "equal"), ({"clips_train": True, "clips": True}, "clips"),
                     # every keyword combination that exists today reaches what it reaches today
                     ({}, "equal"), ({"clips": True}, "clips"), ({"train": True}, "equal"), ({"clips": True, "train": True}, "equal"),
                     ({"clips": False, "train": True, "clips_train": False}, "equal")):
        del calls[:]
        with pytest.raises(Stop):
            arch.run_video_groups(Model(), vids, None, None, None, **kw)
        assert calls[0] == want, kw


def test_wide_heads_keep_todays_training_grouping(monkeypatch):
    """heads of 448 columns have no variable-length attention: `clips_train` changes nothing at that width"""
    from memory_augmented_vlm_amd.model import llava_arch as arch
    calls = []

    class Stop(Exception):
        pass

    def spy(name):
        def f(*a, **k):
            calls.append(name)
            raise Stop
        return f

    monkeypatch.setattr(arch, "plan_row_batches", spy("equal"))
    monkeypatch.setattr(arch, "plan_clip_batches", spy("clips"))

    def model(hd):
        class A:
            attention_head_size = hd

        class L:
            memory_segment_fusion_attention = A

        class RM:
            layers = [L]

        class Model:
            recurrent_memory_transformer = RM

        return Model()

    vids = [(torch.zeros(9, 196, 8), None), (torch.zeros(17, 196, 8), None)]
    for hd, want in ((448, "equal"), (128, "clips"), (112, "clips")):
        del calls[:]
        with pytest.raises(Stop):
            arch.run_video_groups(model(hd), vids, None, None, None, train=True, clips_train=True)
        assert calls == [want], hd


# ---- step_train_frames: the refusals that come before any device work -------------------------------------------------------------------------
def _projector(hidden, heads):
    from memory_augmented_vlm_amd.model.memory_module.MemoryController import Config, TransformerProjector
    c = Config()
    c.mm_hidden_size, c.mm_intermediate_size, c.mm_num_attention_heads = hidden, 4 * hidden, heads
    c.num_memory_tokens, c.depth, c.mm_dtype = 2, 1, torch.float32
    return TransformerProjector(c)


def test_step_train_frames_refusals_without_a_device():
    from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
    assert callable(BatchedProjector.step_train_frames)
    rm = _projector(256, 2)
    bp = BatchedProjector(rm, 4)
    segs = [torch.zeros(f, 196, 256) for f in (4, 2, 1)]                       # host tensors: no check below may get to them
    bp._mode = "engine"                                                        # what the inference `step` leaves behind
    with pytest.raises(capi.MavlmError, match="started by the inference `step`"):
        bp.step_train_frames(segs)
    bp.reset()
    bp._mode, bp._tragged = "autograd", False                                  # ... and `step_train` without `ragged`
    with pytest.raises(capi.MavlmError, match="without `ragged=True`"):
        bp.step_train_frames(segs)
    bp.reset()
    bp.record_attention_maps = True
    with pytest.raises(capi.MavlmError, match="record_attention_maps"):
        bp.step_train_frames(segs)
    bp.record_attention_maps = False
    with pytest.raises(capi.MavlmError, match="2..4 chunks"):                   # the prefix rule of `step_frames`
        bp.step_train_frames(segs[:1])
    with pytest.raises(capi.MavlmError, match="GPU chunks"):                    # nothing before this line objected
        bp.step_train_frames(segs)
    assert bp._mode is None and bp._tcache == [] and bp.frame_scores == []
    wide = BatchedProjector(_projector(896, 2), 2)                              # 2 heads of 448
    with pytest.raises(capi.MavlmError, match="448"):
        wide.step_train_frames([torch.zeros(3, 196, 896), torch.zeros(2, 196, 896)])
    with pytest.raises(capi.MavlmError, match="GPU chunks"):                    # equal F at that width is `step_train`'s body
        wide.step_train_frames([torch.zeros(3, 196, 896), torch.zeros(3, 196, 896)])
    assert wide._mode is None
