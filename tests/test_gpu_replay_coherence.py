"""-m gpu: the inference paths that REUSE state an eager run would rebuild, against eager runs on the same state and against
torch float64 on the GPU (oracle/torch_path.py):

  * the hipGraph cache behind `prepare_inputs_labels_for_multimodal` (`enable_memory_graphs`) and `GraphedVideoMemory`: a graph
    bakes in the engine's workspace, FIFO ring and packed weight copies, so every change of those (weight updates of every kind,
    `bind_fuser`, a module cast, an engine re-created for a longer chunk) must make the next call equal an eager call;
  * the next chunk's K/V projection on a side stream (`mavlm_project_chunk_ahead`): it must not share the split-K scratch of the
    step it overlaps, and a projection left pending by a discarded video must not be met by a captured step.
Measured errors are printed (-s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd.model import llava_arch as arch
from memory_augmented_vlm_amd.model.memory_module.MemoryController import Config, TransformerProjector
from oracle import memory_path as O
from oracle import torch_path as TP
from gpu_util import rel_l2_t, to_dev
from test_gpu_path import _tiny_host, chain_tol

pytestmark = pytest.mark.gpu
D, T = 1024, 40                   # 32 + 8 frames: two steps, the second with memory evolution


@pytest.fixture(autouse=True)
def _inference_path():
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=None)
def _weights(M, seed):
    return O.make_weights(O.PathConfig(hidden=D, heads=8, mem_tokens=M, depth=2), seed=seed)


class _LM(arch.LlavaMetaForCausalLM):
    """The `*ForCausalLM` side of the graph cache (`_video_tokens` is what `prepare_inputs_labels_for_multimodal` calls)."""

    def __init__(self, model):
        self.model = model

    def get_model(self):
        return self.model


def _prompts():
    g = torch.Generator(device="cpu").manual_seed(5)
    return (torch.randn((10, D), generator=g).to("cuda").bfloat16(), torch.randn((9, D), generator=g).to("cuda").bfloat16())


def _reference_tokens(model, x, idx, M, dtype):
    """Fused memory rows of the token block (fuser(cat(memory_cache)) + type row 0) by the torch restatement of the reference, in
    `dtype` on the GPU, from the model's current (16-bit) parameters and the PE-added frames of the same precision (float64: exact
    sum of the two 16-bit operands)."""
    cfg = O.PathConfig(hidden=D, heads=8, mem_tokens=M, depth=2)
    p = {k: v.detach().to(dtype) for k, v in model.state_dict().items()
         if k.startswith((TP.PFX + ".", "memory_fuser.", "token_type_embedding."))}
    tab = model.positional_encoding.table().to(x.dtype)[idx.to("cuda")]
    xpe = x.to(dtype) + tab.to(dtype)[:, None, :]
    cache = TP.run_steps(p, cfg, [xpe[0:32], xpe[32:T]])
    return TP.fuse(p, cache)


def _oracle_gate(model, x, idx, M, got, a, b, label):
    """The memory rows against torch float64; the bound is chain_tol of the distance the reference's own bf16 run (the same torch
    restatement in bfloat16) has from float64.  Returns the bound (for the non-vacuity checks of the caller)."""
    ref = _reference_tokens(model, x, idx, M, torch.float64)
    floor = rel_l2_t(_reference_tokens(model, x, idx, M, torch.bfloat16), ref)
    err = rel_l2_t(got[a:b], ref)
    print(f"[M={M} {label}] memory rows vs float64: {err:.2e}, reference bf16 run {floor:.2e}")
    assert err < chain_tol(floor), (err, floor)
    return ref, chain_tol(floor)


def _mutate(case, model, M):
    rm = model.recurrent_memory_transformer
    g = torch.Generator(device="cpu").manual_seed(7)
    if case == "ln_weight":                           # 1: an fp32 LayerNorm copy of the engine
        rm.layers[1].residual.layernorm.weight.mul_(1.5)
    elif case == "v_bias":                            # 2: the packed K/V bias copy (a K bias would not move the softmax)
        b = rm.layers[0].memory_segment_fusion_attention.v_proj.bias
        b.add_((torch.randn(b.shape, generator=g) * 0.5).to(b.device, b.dtype))
    elif case == "fuser_bias":                        # 3: the fuser's second bias (folded with type row 0 into one fp32 copy)
        b = model.memory_fuser[2].bias
        b.add_((torch.randn(b.shape, generator=g) * 0.5).to(b.device, b.dtype))
    elif case == "load_state_dict":                   # 4
        sd = model.state_dict()
        for k, v in _weights(M, 1502).items():
            if k in sd and k != "positional_encoding.frame_embed":
                sd[k] = torch.from_numpy(np.ascontiguousarray(v))
        model.load_state_dict(sd)
    elif case == "zero_data_copy":                    # 5: DeepSpeed ZeRO-1/2 write-back: neither _version nor the pointer moves
        w1 = _weights(M, 1503)
        model.train()
        for k, p_ in model.named_parameters():
            if k in w1 and k.startswith("recurrent_memory_transformer."):
                v0, ptr = p_._version, p_.data_ptr()
                p_.data.copy_(torch.from_numpy(w1[k]).to(p_.dtype))
                assert p_._version == v0 and p_.data_ptr() == ptr
        model.eval()
    elif case == "new_fuser":                         # 6
        torch.manual_seed(1506)
        f = arch.MemoryFuserMLP(D).to("cuda").to(torch.bfloat16).eval()
        model.memory_fuser = f
        rm.bind_fuser(f, model.token_type_embedding)
    elif case == "half_then_bf16":                    # 7: same dtype in the cache key, every tensor and the engine new
        model.half()
        model.bfloat16()
    elif case == "longer_chunk":                      # 8: engine() re-creates the engine for a 40-frame chunk
        eng = rm._engine
        mp, fp = _prompts()
        arch.video_memory_tokens(model, _frames(), torch.arange(T), mp, fp, model.image_newline, chunk=64)
        assert rm._engine is not eng and rm._engine.c.max_chunk_frames == T
    else:
        raise AssertionError(case)


def _frames():
    return to_dev(O.bf16_round(O.hash_normal_like((T, 196, D), 1500)))


MUTATIONS = ["ln_weight", "v_bias", "fuser_bias", "load_state_dict", "zero_data_copy", "new_fuser", "half_then_bf16",
             "longer_chunk"]


@pytest.mark.parametrize("case", MUTATIONS)
@pytest.mark.parametrize("M", [8, 64])
def test_graph_cache_equals_eager_after_every_state_change(M, case):
    """`enable_memory_graphs`: eager, capture, replay (a cache hit: the same graph object) of one video shape; then one change of
    the state a graph bakes in.  The next call through the cache equals an eager call on the changed state bit for bit (tokens
    and `memory_cache`); for the weight updates the tokens differ from the ones before; for 1, 4, 5 they pass the float64 gate
    with the new weights (eager and graph are not equally wrong); and replays resume: the second call after the change is a
    cache hit again.  M = 64: the fused Residual kernel and the stream-K attention run, most fp32 copies are live."""
    model, _ = _tiny_host(O.PathConfig(hidden=D, heads=8, mem_tokens=M, depth=2), _weights(M, 1501))
    lm = _LM(model)
    lm.enable_memory_graphs(2)
    rm = model.recurrent_memory_transformer
    x, idx = _frames(), torch.arange(T)
    mp, fp = _prompts()
    key = (T, tuple(range(T)), True, torch.bfloat16, x.device.index)
    a, b = 10, 10 + 2 * M * 196

    def through_cache():
        out = lm._video_tokens(model, x, idx, mp, fp, True)
        return out, [c.clone() for c in rm.memory_cache]

    def eager():
        cap, lm._mem_graph_capacity = lm._mem_graph_capacity, 0
        try:
            out = lm._video_tokens(model, x, idx, mp, fp, True)
        finally:
            lm._mem_graph_capacity = cap
        return out, [c.clone() for c in rm.memory_cache]

    first, _ = through_cache()                        # eager (first occurrence)
    assert key not in lm._mem_graphs
    second, _ = through_cache()                       # captures
    g0 = lm._mem_graphs[key]
    before, _ = through_cache()                       # replays
    assert lm._mem_graphs[key] is g0 and len(lm._mem_graphs) == 1
    assert torch.equal(first, second) and torch.equal(second, before)

    _mutate(case, model, M)
    got, got_cache = through_cache()
    g1 = lm._mem_graphs[key]
    assert g1 is not g0                               # the stale graph was dropped and captured again
    want, want_cache = eager()
    assert torch.equal(got, want)
    assert len(got_cache) == len(want_cache) == 2 and all(torch.equal(u, v) for u, v in zip(got_cache, want_cache))
    again, _ = through_cache()                        # replays resume: a hit on the new graph
    assert lm._mem_graphs[key] is g1 and torch.equal(again, want)
    if case in MUTATIONS[:5]:
        assert not torch.equal(got[a:b], before[a:b])
    if case in ("ln_weight", "load_state_dict", "zero_data_copy"):
        ref, tol = _oracle_gate(model, x, idx, M, got, a, b, case)
        assert rel_l2_t(before[a:b], ref) > 4 * tol   # the pre-change tokens fail it: the gate tells the two apart


@pytest.mark.parametrize("case", ["ln_weight", "half_then_bf16"])
@pytest.mark.parametrize("slot", ["model", "replica"])
def test_standalone_graph_refuses_a_stale_replay(slot, case):
    """`GraphedVideoMemory` on the model's own engine and on a replica (default): after an in-place LayerNorm update or a
    cast round trip `__call__` raises MavlmError naming the stale state instead of replaying; a new instance equals eager."""
    M = 8
    model, _ = _tiny_host(O.PathConfig(hidden=D, heads=8, mem_tokens=M, depth=2), _weights(M, 1501))
    x, idx = _frames(), torch.arange(T)
    mp, fp = _prompts()
    g = arch.GraphedVideoMemory(model, T, idx, slot=model if slot == "model" else None)
    eager0, _ = arch.video_memory_tokens(model, x, idx, mp, fp, model.image_newline)
    assert torch.equal(g(x, mp, fp, model.image_newline), eager0)
    _mutate(case, model, M)
    with pytest.raises(capi.MavlmError, match="stale graph.*(re-packed|re-created|replaced)"):
        g(x, mp, fp, model.image_newline)
    eager1, _ = arch.video_memory_tokens(model, x, idx, mp, fp, model.image_newline)
    eager1 = eager1.clone()
    g2 = arch.GraphedVideoMemory(model, T, idx, slot=model if slot == "model" else None)
    assert torch.equal(g2(x, mp, fp, model.image_newline), eager1)
    if case == "ln_weight":
        assert not torch.equal(eager1, eager0)


# ------------------------------------------------------------------------------- next chunk's K/V projection on a side stream
W7 = O.PathConfig(hidden=3584, heads=8, mem_tokens=8, depth=1)       # 8 heads of 448, the reference's 8 memory tokens


@functools.lru_cache(maxsize=1)
def _projector_7b_depth1():
    """A depth-1 projector at the OneVision-7B width (`LlavaMetaModel` hard-codes depth 2, where the chunk K/V GEMM never splits):
    torch's own initialisation, LayerNorm affines perturbed, bf16 on the GPU."""
    c = Config()
    c.mm_hidden_size, c.mm_intermediate_size, c.mm_num_attention_heads = W7.hidden, W7.inter, W7.heads
    c.num_memory_tokens, c.patch_size, c.depth, c.mm_layer_norm_eps, c.mm_dtype = W7.mem_tokens, W7.patches, 1, W7.eps, torch.float32
    torch.manual_seed(1600)
    rm = TransformerProjector(c).eval()
    for n, p_ in rm.named_parameters():
        if "layernorm" in n:
            p_.copy_(torch.randn(p_.shape) * 0.1 + (1.0 if n.endswith("weight") else 0.0))
    return rm.to("cuda").to(torch.bfloat16)


def test_projection_ahead_leaves_the_steps_split_scratch_alone():
    """Deterministic: the split-K scratch the GEMMs of a step share (layout entries 10-11) is filled with a sentinel, a 1-frame
    chunk is projected ahead (its GEMM splits into 3 planes at this width), and after a synchronisation the region is unchanged.
    The projection's own scratch (entries 12-13) did receive its planes."""
    rm = _projector_7b_depth1()
    rm.memory_cache = []
    eng = rm.engine(torch.device("cuda", torch.cuda.current_device()), torch.bfloat16)
    offs = (ctypes.c_size_t * 14)()
    capi.check(capi.lib().mavlm_workspace_layout(eng.c, offs, 14), "mavlm_workspace_layout")
    b0 = eng.workspace_base_offset
    shared = eng.workspace[b0 + offs[10]:b0 + offs[10] + offs[11]]
    own = eng.workspace[b0 + offs[12]:b0 + offs[12] + offs[13]]
    assert offs[11] > 0 and offs[13] >= 4 * capi.lib().mavlm_linear_ws_floats(196, 7168, 3584, capi.EPI_BIAS, 7168) > 0
    seg = to_dev(O.bf16_round(O.hash_normal_like((1, 196, W7.hidden), 1601)))
    torch.cuda.synchronize()
    shared.fill_(0xA5)
    own.fill_(0xA5)
    torch.cuda.synchronize()
    rm.project_ahead(seg)
    torch.cuda.synchronize()
    assert bool((shared == 0xA5).all()), "the projection made ahead wrote into the step's split-K scratch"
    assert not bool((own == 0xA5).all())
    rm.memory_cache = []


def test_projection_ahead_at_depth_one_equals_the_plain_loop_and_float64():
    """End to end where `ahead_ok()` turns the projection on by itself and both GEMMs split: three back-to-back 9-frame videos in
    chunks of 4 + 4 + 1, `project_ahead(next chunk)` before each step as `video_memory_tokens` does.  Memory and frame scores equal
    the same loop without it bit for bit, every announced chunk is a prefetch hit, and the memory passes the float64 gate."""
    rm = _projector_7b_depth1()
    assert rm.ahead_ok()                                                # automatic, nothing forced
    vids = [to_dev(O.bf16_round(O.hash_normal_like((9, 196, W7.hidden), 1610 + v))) for v in range(3)]
    bounds = (0, 4, 8, 9)
    lib = capi.lib()

    def run(ahead):
        outs = []
        for v in vids:
            rm.memory_cache = []
            segs = [v[bounds[i]:bounds[i + 1]] for i in range(3)]
            for i, s_ in enumerate(segs):
                if ahead and i + 1 < len(segs):
                    rm.project_ahead(segs[i + 1])
                rm(s_)
            outs.append(([c.clone() for c in rm.memory_cache], [s_.clone() for s_ in rm.frame_attn_scores[-3:]]))
        return outs

    plain = run(False)
    h0 = lib.mavlm_prefetch_hits(rm._engine.ctx)
    ahead = run(True)
    torch.cuda.synchronize()
    assert lib.mavlm_prefetch_hits(rm._engine.ctx) - h0 == 3 * 2
    for (mc, sc), (mp_, sp_) in zip(ahead, plain):
        assert all(torch.equal(u, w) for u, w in zip(mc, mp_)) and all(torch.equal(u, w) for u, w in zip(sc, sp_))
    p = {TP.PFX + "." + k: v.detach() for k, v in rm.state_dict().items()}
    for v, (mc, _) in zip(vids, ahead):
        segs = [v[bounds[i]:bounds[i + 1]] for i in range(3)]
        ref = TP.run_steps({k: t.double() for k, t in p.items()}, W7, segs)
        ref16 = TP.run_steps(p, W7, segs)
        floor = rel_l2_t(torch.stack(ref16), torch.stack(ref))
        err = rel_l2_t(torch.stack(mc), torch.stack(ref))
        print(f"[7B width, depth 1] memory vs float64: {err:.2e}, reference bf16 run {floor:.2e}")
        assert err < chain_tol(floor), (err, floor)


# ------------------------------------------------------------------------------------ a capture after a discarded projection
def _discard_two_projections(rm, x):
    """A video abandoned after announcing chunks: the projection for step 1 sits in buffer 1, the one for step 2 in buffer 0 -
    both discarded by `memory_cache = []`, both possibly still running on the side stream."""
    rm.memory_cache = []
    rm.project_ahead(x[32:64])
    rm(x[0:32])
    rm.project_ahead(x[64:70])
    rm.memory_cache = []


def test_capture_refuses_a_step_over_a_pending_projection():
    """A step captured into a graph cannot wait for a projection still pending in its K/V buffer (the event belongs to work
    outside the graph): it raises MavlmError (MAVLM_E_STATE) instead of capturing a projection into a buffer the side stream
    may still be writing.  The next eager video waits for it and equals the reference."""
    model, _ = _tiny_host(O.PathConfig(hidden=D, heads=8, mem_tokens=8, depth=2), _weights(8, 1501))
    rm = model.recurrent_memory_transformer
    x = to_dev(O.bf16_round(O.hash_normal_like((70, 196, D), 1700)))
    idx = torch.arange(70)
    mp, fp = _prompts()
    prev = arch.PROJECT_AHEAD
    try:
        arch.PROJECT_AHEAD = False
        want = arch.video_memory_tokens(model, x, idx, mp, fp, model.image_newline)[0].clone()
        arch.PROJECT_AHEAD = True
        _discard_two_projections(rm, x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(capi.MavlmError, match="inside a graph capture"):
            with torch.cuda.graph(graph, stream=side):
                rm(x[0:32])
        del graph
        torch.cuda.current_stream().wait_stream(side)
        got = arch.video_memory_tokens(model, x, idx, mp, fp, model.image_newline)[0]
        assert torch.equal(got, want)
    finally:
        arch.PROJECT_AHEAD = prev


def test_graphed_video_memory_after_a_discarded_projection():
    """`GraphedVideoMemory` on the model's engine right after a discarded projection: its eager warm-up waits for the pending
    projection, so the capture meets none; it builds and replays equal to eager."""
    model, _ = _tiny_host(O.PathConfig(hidden=D, heads=8, mem_tokens=8, depth=2), _weights(8, 1501))
    rm = model.recurrent_memory_transformer
    x = to_dev(O.bf16_round(O.hash_normal_like((70, 196, D), 1701)))
    idx = torch.arange(70)
    mp, fp = _prompts()
    prev = arch.PROJECT_AHEAD
    try:
        arch.PROJECT_AHEAD = True
        _discard_two_projections(rm, x)
        g = arch.GraphedVideoMemory(model, 70, idx, slot=model)
        out = g(x, mp, fp, model.image_newline).clone()
        want = arch.video_memory_tokens(model, x, idx, mp, fp, model.image_newline)[0]
        assert torch.equal(out, want)
    finally:
        arch.PROJECT_AHEAD = prev
