"""CPU (-m "not gpu") tests of clip row batches under autograd at heads of 448 columns: the binding of the variable-length 448
attention backward (`mavlm_attention_bwd_hd_batch_varlen`), its refusals (every one before any launch: none needs a device), the
process-wide Python switch (`ops.set_attention_hd_varlen_train`, off by default), the grouping of `run_video_groups` and the
refusals of `step_train_frames` with the switch on and off."""
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

NEW = "mavlm_attention_bwd_hd_batch_varlen"


@pytest.fixture(scope="module")
def built_lib():
    return pkg.build_library()


def _S(*v):
    return (capi.i32 * len(v))(*v)


def _off(*v):
    return (ctypes.c_int64 * len(v))(*v)


class _switch:
    """the process-wide switch of this file, put back on the way out"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.before = ops.attention_hd_varlen_train()
        ops.set_attention_hd_varlen_train(self.on)

    def __exit__(self, *exc):
        ops.set_attention_hd_varlen_train(self.before)


def test_new_export_is_declared_and_bound(built_lib):
    hdr = open(os.path.join(ROOT, "include", "mavlm.h")).read()
    l = ctypes.CDLL(built_lib)
    assert NEW in capi.SIGNATURES and hasattr(l, NEW)
    assert re.search(r"\bint %s\(" % NEW, hdr)
    assert re.search(r"#define MAVLM_ABI_VERSION 3\b", hdr) and capi.lib().mavlm_abi_version() == 3
    # the header's parameter list and the ctypes table agree in length, and with the 128 export's
    decl = re.search(r"\bint %s\(([^;]*)\);" % NEW, hdr).group(1)
    assert len(decl.split(",")) == len(capi.SIGNATURES[NEW][1]) == 28
    assert capi.SIGNATURES[NEW] == capi.SIGNATURES["mavlm_attention_bwd_batch_varlen"]


def test_wrapper_and_autograd_form_exist():
    assert callable(ops.attention_bwd_hd_batch_varlen)
    want = list(inspect.signature(ops.attention_bwd_batch_varlen).parameters)
    want.remove("head_dim")
    assert list(inspect.signature(ops.attention_bwd_hd_batch_varlen).parameters) == want
    # the wrapper refuses CPU tensors (no fallback) before anything else
    q = torch.zeros(392, 896, dtype=torch.bfloat16)
    kv = torch.zeros(104, 896, dtype=torch.bfloat16)
    with pytest.raises(capi.MavlmError):
        ops.attention_bwd_hd_batch_varlen(q, kv, kv, q, q, torch.zeros(4, 196), 2, (40, 64))
    # AttentionFn with key counts: heads of 128 and of 448, nothing else
    with pytest.raises(capi.MavlmError, match="128 or 448"):
        ag.AttentionFn.apply(q, kv, kv, 2, 0.1, 256, False, 1, (40, 64))


def test_varlen_backward_refusals_without_a_device(built_lib):
    lib = capi.lib()
    P, ld, R = 4096, 896, 196

    def bwd(S, off, nb, doff=None, H=None, hd=448, ldk=ld, ldv=ld, lddk=ld, lddv=ld, dq=P, dk=P, dv=P, q=P, dtype=capi.BF16):
        return getattr(lib, NEW)(q, ld, P, ldk, P, ldv, P, ld, P, ld, P, P, dq, ld, dk, lddk, dv, lddv, R, _S(*S), _off(*off),
                                 _off(*(off if doff is None else doff)), 2 * nb if H is None else H, 0.1, nb, hd, dtype, None)

    two = ([64, 64], [0, 64 * ld], 2)
    S17, off17 = [64] * 17, [64 * ld * b for b in range(17)]
    assert bwd(S17, off17, 17) == capi.E_ARG                                  # more videos than the by-value arrays hold
    assert bwd([64], [0], 0) == capi.E_ARG
    assert bwd(*two, H=3) == capi.E_ARG                                       # H % nb
    assert bwd(*two, q=None) == capi.E_ARG                                    # a null required pointer
    assert bwd(*two, dtype=7) == capi.E_ARG
    assert bwd([64, 0], [0, 64 * ld], 2) == capi.E_ARG                        # S[b] < 1
    assert bwd([64, 64], [0, 63 * ld], 2, doff=[0, 64 * ld]) == capi.E_ARG    # video 1's keys start inside video 0's
    assert bwd(*two, doff=[0, 63 * ld]) == capi.E_ARG                         # video 1's key gradients start inside video 0's
    assert bwd([20, 40, 980], [0, 20 * ld, 60 * ld], 3, doff=[0, 20 * ld, 59 * ld]) == capi.E_ARG
    # ranges that are disjoint by three of the four strides and overlap by the fourth
    wide = 2 * ld
    assert bwd(*two, ldv=wide) == capi.E_ARG
    assert bwd(*two, ldk=wide) == capi.E_ARG
    assert bwd(*two, lddk=wide) == capi.E_ARG
    assert bwd(*two, lddv=wide) == capi.E_ARG
    assert bwd([64, 64], [0, 64 * ld + 4], 2, doff=[0, 64 * ld]) == capi.E_ARG            # alignment of an offset
    assert bwd(*two, doff=[0, 64 * ld + 4]) == capi.E_ARG
    assert bwd(*two, doff=[0, -8]) == capi.E_ARG
    assert bwd([64, 64], [-8, 64 * ld], 2, doff=[0, 64 * ld]) == capi.E_ARG
    assert bwd(*two, ldk=ld + 4) == capi.E_ARG                                # stride alignment
    assert bwd(*two, lddk=ld + 2) == capi.E_ARG
    assert bwd(*two, ldk=ld - 8) == capi.E_ARG                                # narrower than one video's heads (2 x 448)
    assert bwd(*two, lddv=ld - 8) == capi.E_ARG
    assert bwd(*two, q=P + 8) == capi.E_ARG                                   # an input that is not 16-byte aligned
    assert bwd(*two, dk=P + 4) == capi.E_ARG                                  # a gradient pointer that is not 8-byte aligned
    assert bwd(*two, dq=P + 4) == capi.E_ARG
    for hd in (128, 256, 0):
        assert bwd(*two, hd=hd) == capi.E_SHAPE, hd
    # the order of the checks: the width-free argument checks, then the shape, then everything that needs the width
    assert bwd(*two, hd=128, H=3) == capi.E_ARG
    assert bwd(*two, hd=128, ldk=ld + 4) == capi.E_SHAPE
    assert bwd([64, 0], [0, 64 * ld], 2, hd=128) == capi.E_SHAPE
    # a video whose keys exceed the kernel's 32-bit offsets (one tile past the end included)
    big = -(-(1 << 31) // (2 * ld)) - 64                                      # the first count with (S + 64) * ld * 2 >= 2^31
    assert ((big + 64) * ld * 2 >= 1 << 31) and ((big + 63) * ld * 2 < 1 << 31)
    assert bwd([64, big], [0, 64 * ld], 2) == capi.E_ARG
    # the 128 export keeps refusing this width
    assert lib.mavlm_attention_bwd_batch_varlen(P, ld, P, ld, P, ld, P, ld, P, ld, P, P, P, ld, P, ld, P, ld, R, _S(64, 64),
                                                _off(0, 64 * ld), _off(0, 64 * ld), 4, 0.1, 2, 448, capi.BF16, None) == capi.E_SHAPE


# ---- the switch and the grouping ---------------------------------------------------------------------------------------------------------
def test_switch_defaults_to_off_and_reads_back():
    assert ops.attention_hd_varlen_train() is False
    try:
        ops.set_attention_hd_varlen_train(True)
        assert ops.attention_hd_varlen_train() is True
        ops.set_attention_hd_varlen_train(0)
        assert ops.attention_hd_varlen_train() is False
        ops.set_attention_hd_varlen_train(1)
        assert ops.attention_hd_varlen_train() is True
    finally:
        ops.set_attention_hd_varlen_train(False)
    assert ops.attention_hd_varlen_train() is False


def test_switch_routes_wide_heads_to_the_clip_planner(monkeypatch):
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
    for on, hd, kw, want in ((True, 448, {"train": True, "clips_train": True}, "clips"),
                             (False, 448, {"train": True, "clips_train": True}, "equal"),
                             (True, 128, {"train": True, "clips_train": True}, "clips"),
                             (False, 128, {"train": True, "clips_train": True}, "clips"),
                             (True, 112, {"train": True, "clips_train": True}, "clips"),
                             # the switch alone regroups nothing: it needs `train` and `clips_train`
                             (True, 448, {"train": True}, "equal"),
                             (True, 448, {"clips_train": True}, "equal"),
                             # a width with no variable-length kernel at all
                             (True, 256, {"train": True, "clips_train": True}, "equal")):
        del calls[:]
        with _switch(on):
            with pytest.raises(Stop):
                arch.run_video_groups(model(hd), vids, None, None, None, **kw)
        assert calls == [want], (on, hd, kw)
    assert ops.attention_hd_varlen_train() is False
    assert list(inspect.signature(arch.run_video_groups).parameters)[-1] == "clips_train"        # no new keyword: the switch is global


# ---- step_train_frames: the refusals that come before any device work ---------------------------------------------------------------------
def _projector(hidden, heads):
    from memory_augmented_vlm_amd.model.memory_module.MemoryController import Config, TransformerProjector
    c = Config()
    c.mm_hidden_size, c.mm_intermediate_size, c.mm_num_attention_heads = hidden, 4 * hidden, heads
    c.num_memory_tokens, c.depth, c.mm_dtype = 2, 1, torch.float32
    return TransformerProjector(c)


def test_step_train_frames_at_448_with_the_switch_on_and_off():
    from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
    wide = BatchedProjector(_projector(896, 2), 2)                              # 2 heads of 448
    segs = [torch.zeros(3, 196, 896), torch.zeros(2, 196, 896)]                 # host tensors: no check below may get to them
    with _switch(False):
        with pytest.raises(capi.MavlmError, match="448"):
            wide.step_train_frames(segs)
        assert wide._mode is None
    with _switch(True):
        with pytest.raises(capi.MavlmError, match="GPU chunks"):                # nothing before this line objected
            wide.step_train_frames(segs)
        assert wide._mode is None and wide._tcache == [] and wide.frame_scores == []
    with pytest.raises(capi.MavlmError, match="448"):                           # ... and the switch is back off
        wide.step_train_frames(segs)
    assert wide._mode is None
