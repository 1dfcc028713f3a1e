"""CPU (-m "not gpu") tests of the variable-length forward for heads of 448 columns (`mavlm_attention_hd_batch_varlen`) and its
switch in the clip step (`mavlm_set_attention_hd_varlen`, off by default): the binding of the two exports, the hook's default, the
refusals that need no device - the list of tests/test_clip_batch_cpu.py at W = 2 * 448 - and that the narrow export still refuses
448."""
import ctypes
import os
import re

import pytest
import torch

import memory_augmented_vlm_amd as pkg
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from conftest import ROOT

NEW = ("mavlm_attention_hd_batch_varlen", "mavlm_set_attention_hd_varlen")


@pytest.fixture(scope="module")
def built_lib():
    path = pkg.build_library()
    l = ctypes.CDLL(path)
    assert all(hasattr(l, name) for name in NEW), "the library lacks the exports this file is about"
    return path


def _S(*v):
    return (capi.i32 * len(v))(*v)


def _off(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_new_exports_are_declared_and_bound(built_lib):
    hdr = open(os.path.join(ROOT, "include", "mavlm.h")).read()
    l = ctypes.CDLL(built_lib)
    for name in NEW:
        assert name in capi.SIGNATURES and hasattr(l, name)
        assert re.search(r"\bint %s\(" % name, hdr)
    # the parameter list of the narrow export
    assert capi.SIGNATURES["mavlm_attention_hd_batch_varlen"] == capi.SIGNATURES["mavlm_attention_batch_varlen"]
    assert re.search(r"#define MAVLM_ABI_VERSION 3\b", hdr) and capi.lib().mavlm_abi_version() == 3


def test_hook_is_off_by_default_and_round_trips(built_lib):
    """the switch is read through the global the hook writes (every test that flips it puts it back, so what this process shows
    is the default); bad values are refused and change nothing"""
    lib = capi.lib()
    g = ctypes.c_int.in_dll(lib, "g_mavlm_attn_hd_varlen")
    assert g.value == 0
    try:
        assert lib.mavlm_set_attention_hd_varlen(1) == 0 and g.value == 1
        assert lib.mavlm_set_attention_hd_varlen(2) == capi.E_ARG and lib.mavlm_set_attention_hd_varlen(-1) == capi.E_ARG
        assert g.value == 1
        assert lib.mavlm_set_attention_hd_varlen(0) == 0 and g.value == 0
        ops.set_attention_hd_varlen(True)
        assert g.value == 1
        ops.set_attention_hd_varlen(False)
        assert g.value == 0
    finally:
        assert lib.mavlm_set_attention_hd_varlen(0) == 0


def test_wide_varlen_operator_refusals_without_a_device(built_lib):
    lib = capi.lib()
    P, ld, R = 4096, 2 * 448, 196

    def fwd(S, off, nb, H=None, hd=448, ldk=ld, q=P, o=P):
        return lib.mavlm_attention_hd_batch_varlen(q, ld, P, ldk, P, ld, o, ld, None, R, _S(*S), _off(*off), 2 * nb if H is None else H,
                                                   0.1, nb, hd, capi.BF16, None)

    S17, off17 = [64] * 17, [64 * ld * b for b in range(17)]
    assert fwd(S17, off17, 17) == capi.E_ARG                                  # more videos than the by-value arrays hold
    assert fwd([64], [0], 0) == capi.E_ARG
    assert fwd([64, 64], [0, 64 * ld], 2, H=3) == capi.E_ARG                  # H % nb
    assert fwd([64, 0], [0, 64 * ld], 2) == capi.E_ARG                        # S[b] < 1
    assert fwd([64, 64], [0, 63 * ld], 2) == capi.E_ARG                       # video 1 starts inside video 0's keys
    assert fwd([40, 64, 980], [0, 40 * ld, 103 * ld], 3) == capi.E_ARG        # video 2 starts on video 1's last row
    assert fwd([64, 64], [0, 64 * ld + 4], 2) == capi.E_ARG                   # alignment
    assert fwd([64, 64], [0, -8], 2) == capi.E_ARG
    assert fwd([64, 64], [0, 64 * ld], 2, ldk=ld + 4) == capi.E_ARG           # stride alignment
    assert fwd([64, 64], [0, 64 * ld], 2, ldk=448) == capi.E_ARG              # a stride shorter than a video's heads
    assert fwd([64, 64], [0, 64 * ld], 2, q=P + 8) == capi.E_ARG              # Q off its 16 bytes
    assert fwd([64, 64], [0, 64 * ld], 2, o=P + 4) == capi.E_ARG              # O off its 8 bytes
    assert lib.mavlm_attention_hd_batch_varlen(None, ld, P, ld, P, ld, P, ld, None, R, _S(64), _off(0), 2, 0.1, 1, 448, capi.BF16,
                                               None) == capi.E_ARG
    # the kernel's 32-bit byte offsets inside ONE video, a 32-key tile behind its ragged last tile included: (S + 64) * ld * 2 < 2^31
    big = -(-(1 << 31) // (2 * ld)) - 64
    assert (big + 64) * ld * 2 >= 1 << 31 > (big - 1 + 64) * ld * 2
    assert fwd([64, big], [0, 64 * ld], 2) == capi.E_ARG                      # a video past the 32-bit reach
    assert fwd([big], [0], 1, H=2) == capi.E_ARG
    for hd in (128, 256, 0):
        assert fwd([64, 64], [0, 64 * ld], 2, hd=hd) == capi.E_SHAPE
    try:                                                                      # the 16-query-wave kernel has no such form
        assert lib.mavlm_set_attention_wide_groups(1) == 0
        assert fwd([64, 64], [0, 64 * ld], 2) == capi.E_SHAPE
    finally:
        assert lib.mavlm_set_attention_wide_groups(0) == 0


def test_the_narrow_export_still_refuses_448(built_lib):
    lib = capi.lib()
    P, ld = 4096, 2 * 448
    assert lib.mavlm_attention_batch_varlen(P, ld, P, ld, P, ld, P, ld, None, 196, _S(64, 64), _off(0, 64 * ld), 4, 0.1, 2, 448,
                                            capi.BF16, None) == capi.E_SHAPE


def test_wrapper_refuses_host_tensors(built_lib):
    q = torch.zeros((2 * 196, 896), dtype=torch.bfloat16)
    kv = torch.zeros((128, 896), dtype=torch.bfloat16)
    with pytest.raises(capi.MavlmError):
        ops.attention_hd_batch_varlen(q, kv, kv, 2, (64, 64))
