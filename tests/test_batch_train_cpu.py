"""Row-batched training, host side (no GPU): the four row-batch entry points of the C ABI refuse bad arguments with the documented
codes before anything is enqueued - no launch is reached, so no device is needed - and the Python layers expose the batch."""
import inspect

import pytest

import memory_augmented_vlm_amd as pkg
from memory_augmented_vlm_amd import _capi as capi

P = 0x10000          # a non-null, 16-byte aligned "pointer": every call below must return before it is dereferenced
R, S, H, W = 200, 260, 6, 256


@pytest.fixture(scope="module")
def lib():
    pkg.build_library()
    return capi.lib()


def _fwd(lib, q=P, k=P, v=P, o=P, H=H, nb=3, head_dim=128, ld=W, kvb=S * W, ws=0, ws_floats=0):
    return lib.mavlm_attention_batch(q, ld, k, ld, v, ld, o, ld, 0, R, S, H, 0.1, ws, ws_floats, nb, kvb, head_dim, capi.BF16, 0)


def _bwd(lib, q=P, do=P, lse=P, delta=P, H=H, nb=3, hd=None, ld=W):
    a = (q, ld, P, ld, P, ld, P, ld, do, ld, lse, delta, P, ld, P, ld, P, ld, R, S, H)
    tail = (0.1, nb, S * ld, S * ld, capi.BF16, 0)
    if hd is None:
        return lib.mavlm_attention_bwd_batch(*a, *tail)
    return lib.mavlm_attention_bwd_hd_batch(*a, hd, *tail)


def test_forward_batch_refuses_bad_arguments(lib):
    assert capi.MAX_BATCH == 64
    for kw in ({"q": 0}, {"k": 0}, {"v": 0}, {"o": 0}, {"nb": 0}, {"nb": -1}, {"nb": capi.MAX_BATCH + 1, "H": 2 * (capi.MAX_BATCH + 1)},
               {"H": 7}, {"H": 0}, {"ld": 128}, {"ld": W + 4}, {"kvb": -8}, {"kvb": S * W + 1}):
        assert _fwd(lib, **kw) == capi.E_ARG, kw
    for hd in (0, -128, 129, 224, 256, 512):
        assert _fwd(lib, head_dim=hd) == capi.E_SHAPE, hd
    # a null pointer / a bad batch wins over the head size: still an argument error
    assert _fwd(lib, q=0, head_dim=256) == capi.E_ARG and _fwd(lib, nb=0, head_dim=256) == capi.E_ARG
    # the workspace query: 0 for anything the operator would refuse
    for args in ((R, S, H, 0, 128), (R, S, 7, 3, 128), (R, S, H, capi.MAX_BATCH + 1, 128), (R, S, H, 3, 256), (0, S, H, 3, 128)):
        assert lib.mavlm_attention_batch_ws_floats(*args) == 0, args
    # a plan that needs a workspace (a single video's small grid splits its keys) is refused without one
    need = lib.mavlm_attention_batch_ws_floats(1568, 6272, 8, 1, 128)
    assert need == lib.mavlm_attention_ws_floats(1568, 6272, 8) and need > 0
    assert lib.mavlm_attention_batch(P, 1024, P, 1024, P, 1024, P, 1024, 0, 1568, 6272, 8, 0.1, 0, 0, 1, 0, 128, capi.BF16, 0) == capi.E_ARG
    # ... and a row batch never takes that split form: where the stacked grid has no stream-K plan it needs none
    for nb in (2, 4):
        sk = lib.mavlm_attention_batch_ws_floats(1568, 6272, 8 * nb, nb, 128)
        info = (capi.C.c_int32 * 4)()
        assert lib.mavlm_attention_plan(1568, 6272, 8 * nb, info) == 0
        assert (sk > 0) == (info[1] > 0), (nb, sk, list(info))


@pytest.mark.parametrize("hd", [None, 448])
def test_backward_batch_refuses_bad_arguments(lib, hd):
    ld = W if hd is None else 2 * 448
    for kw in ({"q": 0}, {"do": 0}, {"lse": 0}, {"delta": 0}, {"nb": 0}, {"nb": -2}, {"nb": capi.MAX_BATCH + 1, "H": 2 * (capi.MAX_BATCH + 1)},
               {"H": 7}, {"H": 0}, {"ld": ld - 8}):
        kw = dict({"ld": ld}, **kw)
        assert _bwd(lib, hd=hd, **kw) == capi.E_ARG, kw
    if hd is not None:
        for bad in (128, 64, 256, 0):
            assert _bwd(lib, hd=bad, ld=ld) == capi.E_SHAPE, bad
        assert _bwd(lib, hd=128, ld=ld, q=0) == capi.E_ARG and _bwd(lib, hd=128, ld=ld, nb=0) == capi.E_ARG


def test_python_layers_take_the_batch():
    from memory_augmented_vlm_amd import _autograd as ag
    from memory_augmented_vlm_amd import _ops as ops
    from memory_augmented_vlm_amd.model import llava_arch as arch
    from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
    assert inspect.signature(ag.AttentionFn.forward).parameters["nb"].default == 1
    assert inspect.signature(ag.attention_block).parameters["nb"].default == 1
    assert inspect.signature(ag.project_kv).parameters["nb"].default == 1
    assert callable(ops.attention_batch) and callable(ops.attention_bwd_batch)
    assert callable(BatchedProjector.step_train) and callable(arch.video_memory_tokens_batched_train)
    names = list(inspect.signature(arch.video_memory_tokens_batched_train).parameters)
    assert names == ["model", "bp", "images", "frame_idx_cpu", "memory_prompt_embeds", "frame_prompt_embeds", "image_newline",
                     "with_frames", "chunk", "fine_frames", "layout"]
