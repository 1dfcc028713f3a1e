"""Video token layouts (newline per grid row, per frame, one, none) without a GPU: the decision table, the row arithmetic of
the Python surface and of the C ABI, and `relayout` - the expectation function of tests/test_gpu_layouts.py - pinned to what the
reference's own prepare_inputs_labels_for_multimodal produced (tests/golden/g11_layouts.npz, make_golden_layouts.py)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd as pkg
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd.model import llava_arch as arch
from conftest import load_golden

P = 196
N_MP, N_FP = len(arch.MEMORY_PROMPT_IDS), len(arch.FRAME_PROMPT_IDS)
# llava_arch.py:567-634 of the reference: (mm_patch_merge_type, mm_newline_position) -> layout
EXPECTED = {"spatial_unpad__one_token": "one_token", "spatial_unpad__grid": "grid", "spatial_unpad__frame": "frame",
            "spatial_unpad__no_token": "no_token", "spatial__one_token": "no_token", "flat__grid": "no_token"}
PERIOD = {"one_token": 0, "no_token": 0, "frame": 196, "grid": 14}


def relayout(block, period, newline):
    """`block` [rows, D] with one `newline` row [D] behind every `period` rows (period 0: the rows as they are).  numpy only, and
    written here on purpose: it is the expectation of the GPU tests and must not call the code under test."""
    if period == 0:
        return block
    assert block.shape[0] % period == 0
    b = block.reshape(-1, period, block.shape[1])
    nl = np.broadcast_to(np.asarray(newline, dtype=block.dtype).reshape(1, 1, -1), (b.shape[0], 1, b.shape[2]))
    return np.concatenate([b, nl], axis=1).reshape(-1, block.shape[1])


def relayout_tokens(one, mem_rows, fine_rows, layout, newline, with_frames=True, n_mp=N_MP, n_fp=N_FP):
    """The token block of `layout` from the "one_token" block [mem prompt ; memory ; newline ; frame prompt ; fine ; newline]
    (llava_arch.py:620-629,729-731) of the same video: each block laid out on its own."""
    def lay(blk):
        if layout == "one_token":
            return np.concatenate([blk, np.asarray(newline, dtype=blk.dtype).reshape(1, -1)])
        return relayout(blk, PERIOD[layout], newline)
    a = n_mp + mem_rows
    parts = [one[:n_mp], lay(one[n_mp:a])]
    if with_frames:
        b = a + 1 + n_fp
        assert one.shape[0] == b + fine_rows + 1
        parts += [one[a + 1:b], lay(one[b:b + fine_rows])]
    else:
        assert one.shape[0] == a + 1
    return np.concatenate(parts)


def closed_form(T, M, layout, with_frames=True):
    """rows per layout, from the table of the reference's branches: N groups of 196 rows become N*196 (+1) / N*197 / N*210"""
    n = min(-(-T // 32), 10)
    blk = {"one_token": lambda g: g * P + 1, "no_token": lambda g: g * P, "frame": lambda g: g * (P + 1),
           "grid": lambda g: g * (P + 14)}[layout]
    return N_MP + blk(n * M) + ((N_FP + blk(min(32, T))) if with_frames else 0)


def c_rows(M, n, n_fine, with_frames, layout, patches=P):
    c = capi.Config(hidden=1024, heads=8, patches=patches, mem_tokens=M, depth=2, inter=4096, cache_cap=10, max_chunk_frames=32,
                    dtype=0, eps=1e-12)
    return capi.lib().mavlm_layout_rows(c, n, n_fine, N_MP, N_FP, 1 if with_frames else 0, capi.LAYOUTS[layout])


def _cfg(name, **kw):
    merge, pos = name.split("__")[:2]
    return types.SimpleNamespace(mm_patch_merge_type=merge, mm_newline_position=pos, **kw)


def test_token_layout_decision_table_and_errors():
    z, meta = load_golden("g11_layouts.npz")
    assert sorted(meta["configs"]) == sorted(EXPECTED)
    for name in meta["configs"]:
        assert arch.token_layout(_cfg(name)) == EXPECTED[name], name
    # defaults of the reference's getattr calls (:562,564): flat / one_token
    assert arch.token_layout(types.SimpleNamespace()) == "no_token"
    assert arch.token_layout(types.SimpleNamespace(mm_patch_merge_type="spatial_unpad")) == "one_token"
    errs = meta["errors"]
    assert errs == {"spatial_unpad__bogus__newline": "ValueError", "bogus__grid__newline": "ValueError",
                    "spatial__grid__nonewline": "AttributeError"}
    with pytest.raises(ValueError, match="Unexpected mm_newline_position: bogus"):
        arch.token_layout(_cfg("spatial_unpad__bogus"))
    with pytest.raises(ValueError, match="Unexpected mm_patch_merge_type: bogus"):
        arch.token_layout(_cfg("bogus__grid"))
    # a layout that needs the newline on a model without one: AttributeError, as the reference; none needed where none is inserted
    assert arch.token_layout(_cfg("spatial__grid")) == "grid"
    with pytest.raises(AttributeError, match="image_newline"):
        arch._require_newline(None, "grid")
    arch._require_newline(None, "no_token")
    with pytest.raises(NotImplementedError, match="add_faster_video"):
        arch.token_layout(_cfg("spatial_unpad__grid", add_faster_video=True))
    assert arch.token_layout(_cfg("spatial_unpad__frame", add_faster_video=True)) == "frame"
    with pytest.raises(ValueError, match="unknown token layout"):
        arch.video_token_rows(8, 8, layout="bogus")


def test_row_counts_python_c_abi_golden_and_closed_forms():
    z, meta = load_golden("g11_layouts.npz")
    for F0 in meta["videos"]:
        T = arch.sample_frame_count(F0)
        n, n_fine = min(-(-T // 32), 10), min(32, T)
        for name in meta["configs"]:
            L = EXPECTED[name]
            want = int(z[f"rows_{name}_{F0}"]) - meta["n_text"]
            assert arch.video_token_rows(T, 8, layout=L) == want, (F0, name)
            assert c_rows(8, n, n_fine, True, L) == want, (F0, name)
    for T in (1, 8, 31, 32, 64, 330):
        for M in (8, 64):
            for L in arch.LAYOUTS:
                for wf in (True, False):
                    n, n_fine = min(-(-T // 32), 10), min(32, T)
                    py = arch.video_token_rows(T, M, with_frames=wf, layout=L)
                    assert py == closed_form(T, M, L, wf) == c_rows(M, n, n_fine, wf, L), (T, M, L, wf)
    assert arch.video_token_rows(64, 8) == arch.video_token_rows(64, 8, layout="one_token") == 10 + 2 * 1568 + 1 + 9 + 32 * 196 + 1
    # `grid` needs a square patch grid; bad layouts and counts are argument errors
    assert c_rows(8, 1, 8, True, "grid", patches=200) == capi.E_SHAPE
    assert c_rows(8, 1, 8, True, "frame", patches=200) == N_MP + 8 * 201 + N_FP + 8 * 201
    c = capi.Config(hidden=1024, heads=8, patches=P, mem_tokens=8, depth=2, inter=4096, cache_cap=10, max_chunk_frames=32,
                    dtype=0, eps=1e-12)
    assert capi.lib().mavlm_layout_rows(c, 1, 8, N_MP, N_FP, 1, 7) == capi.E_ARG
    assert capi.lib().mavlm_layout_rows(c, -1, 8, N_MP, N_FP, 1, 0) == capi.E_ARG
    assert capi.lib().mavlm_layout_rows(None, 1, 8, N_MP, N_FP, 1, 0) == capi.E_ARG
    with pytest.raises(ValueError, match="square"):
        arch.video_token_rows(8, 8, patches=200, layout="grid")


def test_relayout_reproduces_the_reference_maps_and_rows():
    """`relayout` applied to the control's memory and fine blocks gives every golden map and every stored row exactly."""
    z, meta = load_golden("g11_layouts.npz")
    g6, _ = load_golden("g6_glue.npz")
    newline = z["image_newline"]
    assert float(np.abs(newline).min()) > 0
    step, ip, D = meta["rowstep"], meta["image_pos"], meta["D"]
    for F0 in meta["videos"]:
        T = arch.sample_frame_count(F0)
        mem_rows, fine_rows = min(-(-T // 32), 10) * 8 * P, min(32, T) * P
        n_ctl = int(z[f"rows_{meta['control']}_{F0}"])
        # the control output as row INDICES (column 0) next to the values where the fixtures hold them: all 3161 rows of the
        # 8-frame video in g6_glue.npz (row step 1), every 13th row of the 70-frame video
        ctl_idx = np.arange(n_ctl, dtype=np.int32).reshape(-1, 1)
        ctl_val = np.full((n_ctl, D), np.nan, dtype=np.float32)
        if F0 == 8:
            ctl_val[:] = g6["embeds_8"]
        ctl_val[::step] = z[f"embeds_{meta['control']}_{F0}"]
        for name in meta["configs"]:
            L = EXPECTED[name]
            blk = lambda a, nl: np.concatenate([a[:ip], relayout_tokens(a[ip:n_ctl - (meta["n_text"] - ip)], mem_rows, fine_rows,
                                                                        L, nl), a[n_ctl - (meta["n_text"] - ip):]])
            m = blk(ctl_idx, np.array([-1], dtype=np.int32))[:, 0]
            assert m.shape[0] == int(z[f"rows_{name}_{F0}"]), (F0, name)
            np.testing.assert_array_equal(m, z[f"map_{name}_{F0}"], err_msg=f"{F0} {name}")
            vals = blk(ctl_val, newline)[::step]
            want = z[f"embeds_{name}_{F0}"]
            known = ~np.isnan(vals).any(axis=1)
            assert known.sum() >= (len(want) if F0 == 8 else len(want) // 20)
            assert (vals[known].view(np.uint32) == want[known].view(np.uint32)).all(), (F0, name)
            # labels / mask / positions: IGNORE_INDEX over the block, the text labels around it, all ones, 0..L-1
            lab = z[f"labels_{name}_{F0}"]
            assert (lab[:ip] == -100).all() and (lab[ip:-2] == -100).all() and lab[-2:].tolist() == [33, 44]
            assert z[f"mask_{name}_{F0}"].all() and z[f"mask_{name}_{F0}"].shape == lab.shape == m.shape
            np.testing.assert_array_equal(z[f"pos_{name}_{F0}"], np.arange(m.shape[0]))


def test_training_tail_layout_routes_the_newline_gradient():
    """The torch-op layout of the training tail (CPU tensors here): the rows of `relayout`, and autograd gives the newline the
    sum of the upstream gradient over every inserted row."""
    g = torch.Generator().manual_seed(5)
    blk = torch.randn((3 * P, 8), generator=g, dtype=torch.float64)
    for L in arch.LAYOUTS:
        nl = torch.randn((1, 8), generator=g, dtype=torch.float64, requires_grad=True)
        b = blk.clone().requires_grad_(True)
        out = arch._lay_out_block(b, nl if L != "no_token" else None, L, P)
        want = relayout_tokens(np.concatenate([blk.numpy(), nl.detach().numpy()]), 3 * P, 0, L, nl.detach().numpy()[0],
                               with_frames=False, n_mp=0)
        np.testing.assert_array_equal(out.detach().numpy(), want)
        up = torch.randn(out.shape, generator=g, dtype=torch.float64)
        (out * up).sum().backward()
        idx = relayout_tokens(np.arange(3 * P + 1, dtype=np.int64).reshape(-1, 1), 3 * P, 0, L, np.array([-1]), False, n_mp=0)[:, 0]
        is_nl = idx < 0
        if L != "no_token":
            torch.testing.assert_close(nl.grad[0], up[torch.from_numpy(is_nl)].sum(0), rtol=1e-12, atol=1e-12)
        assert torch.equal(b.grad, up[torch.from_numpy(~is_nl)])


def test_new_symbols_bound_and_abi_version():
    l = capi.lib()
    assert l.mavlm_abi_version() == 3
    for name in ("mavlm_fuse_emit_layout", "mavlm_fuse_emit_layout_batch", "mavlm_layout_rows"):
        assert name in capi.SIGNATURES and hasattr(ctypes.CDLL(l._name), name)
    assert (capi.LAYOUT_ONE, capi.LAYOUT_NONE, capi.LAYOUT_FRAME, capi.LAYOUT_GRID) == (0, 1, 2, 3)
    # null handle / output: argument errors before anything is touched
    rows = ctypes.c_int64(0)
    assert l.mavlm_fuse_emit_layout(None, None, None, 0, None, 0, None, 0, None, 1, 3, None, 0, ctypes.byref(rows), None) == capi.E_ARG
    assert l.mavlm_fuse_emit_layout_batch(None, None, None, 0, None, 0, None, 0, None, 1, 3, None, 0, ctypes.byref(rows),
                                          None) == capi.E_ARG
