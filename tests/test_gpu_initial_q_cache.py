"""-m gpu: the Q projection of the initial memory, made once per weight binding (`mavlm_set_cache_initial_q`, default on)
against the projection at every first step (hook off).  The cached Q is the output of the same GEMM on the same operands, so
everything is compared bit for bit.  Engine at hidden 1024 with 8 memory tokens and 2-frame chunks (the Q GEMM is the same code
at every size); that the cache is really used is read from the launch counters: a video that starts with a valid cache
launches exactly one GEMM less."""
import ctypes
import functools

import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from memory_augmented_vlm_amd.model import llava_arch as arch
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector, _Engine
from oracle import memory_path as O
from gpu_util import to_dev
from test_gpu_path import _tiny_host

pytestmark = pytest.mark.gpu
D, M, T, CHUNK = 1024, 8, 4, 2          # two steps per video: formation from the initial memory, then evolution + formation
CFG = O.PathConfig(hidden=D, heads=8, mem_tokens=M, depth=2)


@pytest.fixture(autouse=True)
def _inference_path(request):
    request.addfinalizer(lambda: capi.lib().mavlm_set_cache_initial_q(1))
    with torch.no_grad():
        yield


def _hook(on):
    capi.check(capi.lib().mavlm_set_cache_initial_q(on), "mavlm_set_cache_initial_q")


@functools.lru_cache(maxsize=None)
def _weights():
    return O.make_weights(CFG, seed=1901)


def _model():
    return _tiny_host(CFG, _weights())[0]


def _frames(seed):
    return to_dev(O.bf16_round(O.hash_normal_like((T, 196, D), seed)))


def _prompts():
    g = torch.Generator(device="cpu").manual_seed(5)
    return (torch.randn((10, D), generator=g).to("cuda").bfloat16(), torch.randn((9, D), generator=g).to("cuda").bfloat16())


def _video(model, x):
    """one eager video: (token block, memories, frame scores of its chunks), all copied"""
    rm = model.recurrent_memory_transformer
    n0 = len(rm.frame_attn_scores)
    mp, fp = _prompts()
    toks, _ = arch.video_memory_tokens(model, x, torch.arange(T), mp, fp, model.image_newline, chunk=CHUNK)
    return toks.clone(), [c.clone() for c in rm.memory_cache], [s.clone() for s in rm.frame_attn_scores[n0:]]


def _same(a, b):
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(u, v) for u, v in zip(a[1], b[1])) and \
        all(torch.equal(u, v) for u, v in zip(a[2], b[2]))


def _gemm_launches(fn):
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
    return sum(ln[capi.KERNEL_KINDS.index(k)] for k in ("gemm", "gemm_splitk", "gemm_layernorm"))


def test_two_videos_with_the_cached_q_equal_the_projection_at_every_first_step():
    model = _model()
    xs = [_frames(1910), _frames(1911)]
    _hook(0)
    off = [_video(model, x) for x in xs]
    n_off = _gemm_launches(lambda: _video(model, xs[0]))
    _hook(1)
    on = [_video(model, x) for x in xs]                # the first projects into the cache, the second reads it
    n_on = _gemm_launches(lambda: _video(model, xs[0]))
    assert all(_same(a, b) for a, b in zip(on, off))
    assert not torch.equal(on[0][0], on[1][0])
    assert n_on == n_off - 1, (n_on, n_off)            # the first step's Q GEMM is gone, nothing else changed


def test_row_batch_with_the_cached_q():
    model = _model()
    rm = model.recurrent_memory_transformer
    vids = [[_frames(1920), _frames(1921)], [_frames(1922), _frames(1923)]]
    mp, fp = _prompts()
    bp = BatchedProjector(rm, 2)
    res = {}
    for on in (0, 1):
        _hook(on)
        res[on] = []
        for v in vids:                                 # two consecutive batches through one engine
            toks, info = arch.video_memory_tokens_batched(model, bp, v, torch.arange(T), mp, fp, model.image_newline, chunk=CHUNK)
            res[on].append((toks.clone(), [c.clone() for b in range(2) for c in bp.memory_cache(b)],
                            [s.clone() for s in info["frame_scores"]]))
    assert all(_same(a, b) for a, b in zip(res[1], res[0]))
    assert not torch.equal(res[1][0][0][0], res[1][0][0][1])       # (the two videos of a batch differ)


def test_row_shard_with_the_cached_q():
    """A row shard (q_tokens < M) packs only its rows of the initial memory; its first steps with the cache equal those without."""
    lib = capi.lib()
    rm = _model().recurrent_memory_transformer
    eng = _Engine(rm, torch.device("cuda", torch.cuda.current_device()), torch.bfloat16, CHUNK, shard=(3, 2))
    eng.pack(rm)
    segs = [_frames(1930)[:CHUNK].contiguous(), _frames(1931)[:CHUNK].contiguous()]
    res = {}
    for on in (0, 1):
        _hook(on)
        res[on] = []
        for x in segs:
            capi.check(lib.mavlm_reset(eng.ctx), "mavlm_reset")
            scores = torch.empty(CHUNK, device="cuda", dtype=torch.bfloat16)
            capi.check(lib.mavlm_step(eng.ctx, x.data_ptr(), CHUNK, scores.data_ptr(), 0, ops.stream_ptr()), "mavlm_step")
            res[on].append((eng.mem_ring[0][3:5].clone(), scores))
    for (m1, s1), (m0, s0) in zip(res[1], res[0]):
        assert torch.equal(m1, m0) and torch.equal(s1, s0)
    assert not torch.equal(res[1][0][0], res[1][1][0])


def test_attention_maps_read_the_cached_q():
    model = _model()
    rm = model.recurrent_memory_transformer
    rm.record_attention_maps = True
    res = {}
    for on in (0, 1):
        _hook(on)
        res[on] = []
        for seed in (1940, 1941):
            out = _video(model, _frames(seed))
            maps = list(rm.attention_maps)
            assert len(maps) == T // CHUNK
            res[on].append((out, [m.formation.clone() for m in maps]))
    for (o1, f1), (o0, f0) in zip(res[1], res[0]):
        assert _same(o1, o0) and all(torch.equal(u, v) for u, v in zip(f1, f0))
        assert float(f1[0].abs().sum()) > 0 and bool(torch.isfinite(f1[0]).all())


@pytest.mark.parametrize("what", ["initial_memory", "wq"])
def test_in_place_weight_updates_drop_the_cached_q(what):
    model = _model()
    rm = model.recurrent_memory_transformer
    x = _frames(1950)
    _hook(1)
    _video(model, x)
    before = _video(model, x)                          # (runs on the cached Q)
    if what == "initial_memory":
        rm.initial_memory.mul_(1.5)
    else:
        w = rm.layers[0].memory_segment_fusion_attention.q_proj.weight
        w.add_((torch.randn(w.shape, generator=torch.Generator(device="cpu").manual_seed(9)) * 0.02).to(w.device, w.dtype))
    got = _video(model, x)
    _hook(0)
    rm._engine = None                                  # a fresh engine, projecting at every first step
    rm._memory_cache = []
    want = _video(model, x)
    assert _same(got, want) and not torch.equal(got[0], before[0])


@pytest.mark.parametrize("valid", [False, True])
def test_graph_captured_before_and_after_the_cache_is_valid(valid):
    """A capture that meets an invalid cache keeps the projection inside the graph; one that meets a valid cache reads it.  Both
    replay to the eager result, also after eager videos have filled the cache in between."""
    model = _model()
    idx = torch.arange(T)
    mp, fp = _prompts()
    xs = [_frames(1960), _frames(1961)]
    if valid:
        _hook(1)
        g = arch.GraphedVideoMemory(model, T, idx, slot=model)       # (its eager warm-up projects into the cache)
        replay = lambda x: g(x, mp, fp, model.image_newline).clone()
    else:
        _hook(0)                                       # warm-up without the cache: engine, packing, kernel attributes
        x_s, mp_s, fp_s, nl_s = torch.zeros_like(xs[0]), mp.clone(), fp.clone(), model.image_newline.detach().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            arch.video_memory_tokens(model, x_s, idx, mp_s, fp_s, nl_s)
        torch.cuda.current_stream().wait_stream(side)
        _hook(1)                                       # the cache is on and has never been filled
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, _ = arch.video_memory_tokens(model, x_s, idx, mp_s, fp_s, nl_s)

        def replay(x):
            x_s.copy_(x)
            graph.replay()
            return out.clone()
    first = [replay(x) for x in xs]
    eager = [arch.video_memory_tokens(model, x, idx, mp, fp, model.image_newline)[0].clone() for x in xs]
    again = [replay(x) for x in xs]
    for a, b, c in zip(first, eager, again):
        assert torch.equal(a, b) and torch.equal(c, b)
    assert not torch.equal(eager[0], eager[1])
