"""CPU (-m "not gpu") tests of the attention maps: the argument checks of the C entry points (they run before any launch, so no
GPU is needed), the buffer protocol of a context, the Python surface, and the reference fixture golden/g10_attention_maps.npz."""

import numpy as np
import pytest

import memory_augmented_vlm_amd as pkg
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd.model.memory_module.MemoryController import (AttentionMaps, BatchedProjector, Config,
                                                                            FusedAttentionStats, TransformerProjector)
from oracle import memory_path as O
from conftest import load_golden


@pytest.fixture(scope="module")
def lib():
    pkg.build_library()
    return capi.lib()


def _call(lib, R=300, S=2000, H=2, hd=128, qg=196, kg=196, floats=None, q=4096, k=4096, lse=4096, out=4096, ldq=None, ldk=None,
          dtype=0):
    """mavlm_attention_group_mass on addresses that are never dereferenced: every call here must fail its checks first"""
    need = lib.mavlm_attention_group_mass_floats(R, S, H, qg, kg)
    return lib.mavlm_attention_group_mass(q, H * hd if ldq is None else ldq, k, H * hd if ldk is None else ldk, lse, out,
                                          need if floats is None else floats, R, S, H, hd, 0.088, qg, kg, dtype, None)


def test_group_mass_argument_errors_before_any_launch(lib):
    need = lib.mavlm_attention_group_mass_floats(300, 2000, 2, 196, 196)
    # result [H, 2, 11] first, then one scratch word per (head, key group, row)
    assert need == 2 * 2 * 11 + 2 * 11 * 300
    assert lib.mavlm_attention_group_mass_floats(1568, 6272, 8, 196, 1568) == 8 * 8 * 4 + 8 * 4 * 1568
    assert lib.mavlm_attention_group_mass_floats(0, 2000, 2, 196, 196) == 0
    assert _call(lib, floats=need - 1) == capi.E_ARG                # too small a buffer: an error, never another path
    assert _call(lib, floats=0) == capi.E_ARG
    assert _call(lib, kg=6) == capi.E_SHAPE                         # a lane holds 4 consecutive keys: k_group % 4 == 0
    assert _call(lib, kg=0) == capi.E_SHAPE and _call(lib, qg=0) == capi.E_SHAPE and _call(lib, qg=-3) == capi.E_SHAPE
    assert _call(lib, hd=256) == capi.E_SHAPE and _call(lib, hd=64) == capi.E_SHAPE
    assert _call(lib, q=None) == capi.E_ARG and _call(lib, k=None) == capi.E_ARG
    assert _call(lib, lse=None) == capi.E_ARG and _call(lib, out=None) == capi.E_ARG
    assert _call(lib, R=0) == capi.E_ARG and _call(lib, S=0) == capi.E_ARG and _call(lib, H=0) == capi.E_ARG
    assert _call(lib, ldq=2 * 128 - 8) == capi.E_ARG and _call(lib, ldk=2 * 128 + 4) == capi.E_ARG
    assert _call(lib, dtype=2) == capi.E_ARG
    assert _call(lib, hd=448, floats=need - 1) == capi.E_ARG


def test_maps_buffer_protocol(lib):
    c = capi.Config(hidden=1024, heads=8, patches=196, mem_tokens=8, depth=2, inter=4096, cache_cap=10, max_chunk_frames=32,
                    dtype=0, eps=1e-12)
    H, M, L, F, cap, R = 8, 8, 2, 32, 10, 1568
    n = lib.mavlm_attention_maps_floats(c)
    # per video [depth, H, M, F] + [H, M, cap], then the larger scratch of the two passes (one word per head, key group, row)
    assert n == L * H * M * F + H * M * cap + max(H * F * R, H * cap * R)
    ws = lib.mavlm_workspace_bytes(c)
    h = capi.vp()
    assert lib.mavlm_create(c, h) == 0
    assert lib.mavlm_bind_attention_maps(h, 4096, n - 1) == capi.E_ARG
    assert lib.mavlm_bind_attention_maps(h, 4098, n) == capi.E_ARG      # not a float address
    assert lib.mavlm_bind_attention_maps(h, 4096, n) == 0
    assert lib.mavlm_bind_attention_maps(h, None, 0) == 0               # off again
    assert lib.mavlm_bind_attention_maps(None, 4096, n) == capi.E_ARG
    assert lib.mavlm_workspace_bytes(c) == ws                           # the workspace does not grow
    lib.mavlm_destroy(h)
    b2 = capi.Config(hidden=1024, heads=8, patches=196, mem_tokens=8, depth=2, inter=4096, cache_cap=10, max_chunk_frames=32,
                     dtype=0, eps=1e-12, batch=2)
    assert lib.mavlm_attention_maps_floats(b2) == 2 * (L * H * M * F + H * M * cap) + max(H * F * R, H * cap * R)
    odd = capi.Config(hidden=1024, heads=8, patches=49, mem_tokens=8, depth=2, inter=4096, cache_cap=10, max_chunk_frames=32,
                      dtype=0, eps=1e-12)                                 # patches % 4 != 0
    assert lib.mavlm_attention_maps_floats(odd) == 0
    h2 = capi.vp()
    assert lib.mavlm_create(odd, h2) == 0
    assert lib.mavlm_bind_attention_maps(h2, 4096, 1 << 40) == capi.E_SHAPE
    lib.mavlm_destroy(h2)
    assert lib.mavlm_abi_version() == 3


def test_python_surface_defaults():
    c = Config()
    c.mm_hidden_size, c.mm_intermediate_size, c.mm_num_attention_heads, c.num_memory_tokens = 256, 1024, 2, 2
    proj = TransformerProjector(c)
    assert proj.record_attention_maps is False and proj.attention_maps == []
    proj.attention_maps.append(AttentionMaps(None, None))
    proj.memory_cache = []                                              # the reset of a video clears the list
    assert proj.attention_maps == []
    r = proj.spawn_replica()
    assert r.record_attention_maps is False and r.attention_maps == [] and r.attention_maps is not proj.attention_maps
    bp = BatchedProjector(proj, 2)
    assert bp.record_attention_maps is False and bp.attention_maps == []
    assert callable(FusedAttentionStats.group_mass)
    from memory_augmented_vlm_amd import _ops as ops
    with pytest.raises(capi.MavlmError):                                # no CPU path
        import torch
        ops.attention_group_mass(torch.zeros(4, 128), torch.zeros(4, 128), torch.zeros(1, 4), 1, 4, 4)


def test_golden_maps_fixture():
    """g10: both runs of the reference are there, every fp32 map is a grouping of softmax rows (row sums = P to 1e-5; the
    formation maps of the last layer give the reference's frame scores), and the formation maps are not uniform."""
    z, meta = load_golden("g10_attention_maps.npz")
    H, M, L, Pp = meta["heads"], meta["mem_tokens"], meta["depth"], meta["patches"]
    assert meta["frames"] == [32, 32, 7] and meta["hidden"] == 1024 and (H, M, L, Pp) == (8, 8, 2, 196)
    assert meta["amplitude"] >= 1.0
    for t, F in enumerate(meta["frames"]):
        for run in ("fp32", "bf16"):
            assert z[f"{run}_form_{t}"].shape == (L, H, M, F) and z[f"{run}_form_{t}"].dtype == np.float32
            if t:
                assert z[f"{run}_evo_{t}"].shape == (H, M, t)
            else:
                assert f"{run}_evo_0" not in z.files
        form = z[f"fp32_form_{t}"].astype(np.float64)
        assert np.max(np.abs(form.sum(-1) - Pp)) < 1e-5 * Pp
        assert O.rel_l2(form[-1].sum(axis=(0, 1)) / Pp, z[f"fp32_scores_{t}"]) < 1e-5
        for l in range(L):
            far = O.rel_l2(form[l], np.full_like(form[l], Pp / F))
            assert far >= 0.1 and abs(far - meta["from_uniform_formation"][t * L + l]) < 1e-6
            e = O.rel_l2(z[f"bf16_form_{t}"][l], form[l])
            assert abs(e - meta["envelope_formation"][t][l]) < 1e-9 and 0 < e < 1e-2
        if t:
            evo = z[f"fp32_evo_{t}"].astype(np.float64)
            assert np.max(np.abs(evo.sum(-1) - Pp)) < 1e-5 * Pp
            e = O.rel_l2(z[f"bf16_evo_{t}"], evo)
            assert abs(e - meta["envelope_evolution"][t - 1]) < 1e-9 and 0 < e < 1e-2
