"""Multimodal glue of the memory path on the MI355X HIP engine.

Mirrors the memory-specific parts of the reference's llava/model/llava_arch.py so the HF/LLaVA backbone
(vision tower, mm_projector, Qwen2 LLM - all unchanged PyTorch-ROCm modules) keeps working:

  LlavaMetaModel            builds `recurrent_memory_transformer`, `memory_fuser`, `positional_encoding`,
                            `token_type_embedding` with the reference's names and hard-coded hyper-parameters
                            (llava_arch.py:117-150) - same state-dict keys, so checkpoints load unchanged.
  LlavaMetaForCausalLM      `prepare_inputs_labels_for_multimodal` (8 in / 6 out, llava_arch.py:388-878) for the
                            video path, `get_2dPool`, `encode_images`, `get_synced_dropout_decision`.
  video_memory_tokens       the per-video driver (llava_arch.py:502-557,567-634,705-731) as HIP launches only:
                            PE add -> chunk loop (mavlm_step) -> fuser MLP + type add + prompts/newlines concat
                            (mavlm_fuse_emit_layout) written straight into one token block, in the layout
                            `token_layout(config)` reads from mm_patch_merge_type / mm_newline_position.
  run_video_groups          several videos of one forward (one per sample): equal sampled lengths step together as row batches,
                            each block emitted at its place in the padded inputs_embeds buffer (`VideoPlacement`,
                            mavlm_fuse_emit_layout_batch_to); the reference serves one video per forward (llava_arch.py:436).

Non-video inputs behave as in the reference (round 3): a plain image batch takes the reference's tensor branch (:703,
backbone ops, restated in torch); a list without a video fails as the reference's memory loop does (IndexError); images
beside the video are dropped as the reference drops them.  The anyres / multi-patch merge modes (:630-697) are unreachable
in the reference's memory branch (its feature list only ever holds the memory and the fine frames) and are not restated.
"""
import ctypes
import math
import random
from typing import List, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from .. import _capi as capi
from .. import _ops as ops
from .memory_module.MemoryController import BatchedProjector, Config, TransformerProjector
from .memory_module.position_encoding import TemporalPositionalEncoding
from .memory_module.segment import uniform_segment_variant

IGNORE_INDEX = -100          # llava/constants.py:7
IMAGE_TOKEN_INDEX = -200     # llava/constants.py:8

# Qwen2-tokenizer ids of the two fixed prompts (llava_arch.py:708,714):
# "This is a high-level summary of the video:" / "These are sampled visual frames from the video:"
MEMORY_PROMPT_IDS = (1986, 374, 264, 1550, 11591, 12126, 315, 279, 2766, 25)
FRAME_PROMPT_IDS = (9485, 525, 48876, 9124, 14087, 504, 279, 2766, 25)


class MemoryFuserMLP(nn.Sequential):
    """`memory_fuser` = Linear(D,4D) -> GELU(erf) -> Linear(4D,D) (llava_arch.py:132-136); state-dict keys
    `0.weight, 0.bias, 2.weight, 2.bias` as the reference's nn.Sequential.  forward = two MFMA GEMMs with the
    GELU fused into the first epilogue."""

    def __init__(self, hidden):
        super().__init__(nn.Linear(hidden, hidden * 4), nn.GELU(), nn.Linear(hidden * 4, hidden))

    def forward(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            from .. import _autograd as ag            # training: same kernels as autograd Functions
            return ag.fuser_mlp(self, x)
        x2 = x.reshape(-1, x.shape[-1])
        u = ops.linear(x2, self[0].weight, self[0].bias.float(), capi.EPI_GELU)
        y = ops.linear(u, self[2].weight, self[2].bias.float(), capi.EPI_BIAS)
        return y.reshape(x.shape)


def sample_frame_count(num_frames: int) -> int:
    """F0 -> F  (llava_arch.py:437-445): all frames below 32, else a multiple of 32 and at least 64."""
    if num_frames < 32:
        return num_frames
    return max(64, (num_frames // 32) * 32)


def sample_frame_indices(num_frames: int) -> torch.Tensor:
    """llava_arch.py:451 - same call the reference makes (CPU float32 linspace, truncation)."""
    return torch.linspace(0, num_frames - 1, steps=sample_frame_count(num_frames)).long()


def fine_frame_indices(num_frames: int, want: int = 32) -> torch.Tensor:
    """llava_arch.py:513-522 - rounded, clamped linspace over the sampled frames."""
    n = min(want, num_frames)
    idx = torch.round(torch.linspace(0, num_frames - 1, steps=n)).long()
    return torch.clamp(idx, 0, num_frames - 1)


class LlavaMetaModel:
    """Mixin for the inner model (the class that owns `embed_tokens`).  Vision modules are the backbone's: attach
    `vision_tower`, `mm_projector`, `image_newline` as the host model does."""

    def __init__(self, config):
        super(LlavaMetaModel, self).__init__(config)
        hidden = getattr(config, "hidden_size", 896)
        c = Config()
        c.mm_hidden_size = hidden
        c.mm_hidden_act = "relu"
        c.mm_num_attention_heads = 8
        c.patch_size = 196
        c.mm_attention_probs_dropout_prob = 0.1
        c.mm_layer_norm_eps = 1e-12
        c.mm_hidden_dropout_prob = 0.1
        c.mm_intermediate_size = 4 * hidden
        c.num_memory_tokens = getattr(config, "num_memory_tokens", 8)     # reference constant: 8
        c.depth = 2
        c.mm_dtype = torch.float16
        c.cache_cap = getattr(config, "memory_cache_cap", 10)
        self.recurrent_memory_transformer = TransformerProjector(c)
        self.memory_fuser = MemoryFuserMLP(hidden)
        self.positional_encoding = TemporalPositionalEncoding(
            max_frames=getattr(config, "memory_max_frames", 600), embed_dim=hidden, learnable=False)
        self.token_type_embedding = nn.Embedding(2, hidden)
        self.recurrent_memory_transformer.bind_fuser(self.memory_fuser, self.token_type_embedding)

    def get_vision_tower(self):
        vt = getattr(self, "vision_tower", None)
        return vt[0] if type(vt) is list else vt


_INDEX_CACHE = {}


def _device_indices(idx_cpu: torch.Tensor, device) -> torch.Tensor:
    """int64 index vectors are tiny and repeat across videos of the same length: cache the device copy so the
    steady state has no H2D copy (a pageable copy would wait for the stream to drain)."""
    key = (str(device), idx_cpu.numel(), idx_cpu.numpy().tobytes())
    t = _INDEX_CACHE.get(key)
    if t is None:
        if len(_INDEX_CACHE) > 256:
            _INDEX_CACHE.clear()
        t = idx_cpu.to(device=device, dtype=torch.int64)
        _INDEX_CACHE[key] = t
    return t


LAYOUTS = ("one_token", "no_token", "frame", "grid")


def token_layout(config) -> str:
    """Layout of the video token block for a model config: where the reference puts `image_newline` rows into the memory
    block and into the fine-frame block (llava_arch.py:562-634) -
      "one_token"  one newline behind each block (spatial*_unpad + one_token, :620-629),
      "no_token"   none (flat, :567-569; spatial* + no_token, :631-632; spatial* without unpad + one_token, :623),
      "frame"      one after every 196 rows (add_token_per_frame, :353-357),
      "grid"       one after every 14 rows (add_token_per_grid, :330-351).
    The one place that reads mm_patch_merge_type, mm_newline_position and add_faster_video; raises what the reference raises
    (ValueError, :634 / :701).  `grid` with add_faster_video reads tensors the memory branch never creates: NotImplementedError."""
    merge = getattr(config, "mm_patch_merge_type", "flat")                                  # :562
    pos = getattr(config, "mm_newline_position", "one_token")                              # :564
    if merge == "flat":
        return "no_token"                                                                  # :567-569 (the position is ignored)
    if not merge.startswith("spatial"):
        raise ValueError(f"Unexpected mm_patch_merge_type: {merge}")                       # :701
    if pos == "grid":
        if getattr(config, "add_faster_video", False):
            raise NotImplementedError("memory path: mm_newline_position='grid' with add_faster_video (llava_arch.py:590-601 "
                                      "reads faster-video features the memory branch never creates)")
        return "grid"
    if pos == "frame":
        return "frame"
    if pos == "one_token":
        return "one_token" if "unpad" in merge else "no_token"                             # :623
    if pos == "no_token":
        return "no_token"
    raise ValueError(f"Unexpected mm_newline_position: {pos}")                             # :634


def layout_period(layout: str, patches: int = 196) -> int:
    """Newline period of a layout inside a block: 0 = none inside it ("one_token": one behind it; "no_token": none at all),
    else one newline row after every `period` rows ("frame": a frame's patches; "grid": one row of its square patch grid)."""
    if layout not in LAYOUTS:
        raise ValueError(f"unknown token layout {layout!r}: one of {LAYOUTS}")
    if layout == "frame":
        return patches
    if layout == "grid":
        g = math.isqrt(patches)
        if g * g != patches:
            raise ValueError(f"token layout 'grid' needs a square patch grid, not {patches} patches per frame")
        return g
    return 0


def layout_block_rows(rows: int, layout: str, patches: int = 196) -> int:
    """Rows a block of `rows` feature rows (whole frames) takes in a layout."""
    g = layout_period(layout, patches)
    return rows + (rows // g if g else (1 if layout == "one_token" else 0))


def _require_newline(image_newline, layout):
    """The reference creates `image_newline` only for an *_unpad merge type (llava_arch.py:114) and fails with AttributeError
    where a layout reads it on a model without one; a layout that inserts nothing needs none."""
    if layout != "no_token" and image_newline is None:
        raise AttributeError(f"token layout {layout!r} inserts `image_newline` rows, but the model has no image_newline (the "
                             "reference creates it only when mm_patch_merge_type contains 'unpad', llava_arch.py:114)")


def _newline_ptr(image_newline, layout, device, dtype):
    """(tensor kept alive, device pointer) of the newline row a layout inserts; (None, None) for a layout that inserts nothing"""
    _require_newline(image_newline, layout)
    if layout == "no_token":
        return None, None
    nl = image_newline.to(device=device, dtype=dtype).contiguous()
    return nl, nl.data_ptr()


def video_token_rows(num_frames: int, mem_tokens: int, patches: int = 196, with_frames: bool = True, chunk: int = 32,
                     fine_frames: int = 32, cache_cap: int = 10, n_mem_prompt: int = len(MEMORY_PROMPT_IDS),
                     n_frame_prompt: int = len(FRAME_PROMPT_IDS), layout: str = "one_token") -> int:
    """Rows of the token block video_memory_tokens() produces for a T-frame video (host arithmetic only), so a caller
    can allocate the final sequence once and have the block emitted in place.  `layout`: see token_layout()."""
    n = min(-(-num_frames // chunk), cache_cap)
    rows = n_mem_prompt + layout_block_rows(n * mem_tokens * patches, layout, patches)
    if with_frames:
        rows += n_frame_prompt + layout_block_rows(min(fine_frames, num_frames) * patches, layout, patches)
    return rows


PROJECT_AHEAD = None      # None: automatic (TransformerProjector.ahead_ok), True: wherever the memory rows are few, False: never


def video_memory_tokens(model, image: torch.Tensor, frame_idx_cpu: torch.Tensor, memory_prompt_embeds: torch.Tensor,
                        frame_prompt_embeds: torch.Tensor, image_newline: Optional[torch.Tensor], with_frames: bool = True,
                        chunk: int = 32, fine_frames: int = 32, out: Optional[torch.Tensor] = None, layout: str = "one_token"):
    """Per-video memory path.  `model` owns the four memory sub-modules; `image` = pooled frame tokens [T,196,D]
    on the GPU; `frame_idx_cpu` = original frame indices [T] (host).  Returns (tokens [rows,D], info dict).

    tokens = [mem_prompt ; fused memory (oldest first) ; newline ; frame_prompt ; fine frames ; newline]
    (llava_arch.py:620-629,729-731); with_frames=False reproduces the frame-dropout branch (:720-725).
    `layout` (token_layout(config): "one_token" above, "no_token", "frame", "grid") moves the newlines: none, or one after every
    196 / 14 rows of the memory block and of the fine-frame block (:567-634); the other rows are the same bits in every layout.
    `image_newline` may be None for "no_token".
    `out`: optional contiguous [rows, D] destination (e.g. a slice of the final inputs_embeds buffer)."""
    layout_period(layout, image.shape[1])                                                 # (ValueError for an unknown layout)
    if not image.is_cuda:
        raise capi.MavlmError("video_memory_tokens: frame tokens are not on a GPU (no CPU fallback)")
    pe: TemporalPositionalEncoding = model.positional_encoding
    rm: TransformerProjector = model.recurrent_memory_transformer
    T, P, D = image.shape
    pe.check_indices(frame_idx_cpu)                                                       # ValueError, :73-76
    x = pe(image, _device_indices(frame_idx_cpu, image.device), indices_checked=True)     # :510-511
    fine_cpu = fine_frame_indices(T, fine_frames)                                         # :513-522
    bounds = uniform_segment_variant(T, chunk)                                            # :528
    rm.memory_cache = []                                                                  # :532
    # (few memory tokens: the next chunk's K/V projection - the largest GEMM of a step there - runs on a side stream beside this
    #  chunk's small-grid kernels, TransformerProjector.project_ahead; PROJECT_AHEAD = False switches it off)
    ahead = PROJECT_AHEAD is not False and len(bounds) > 2 and rm.ahead_ok(force=PROJECT_AHEAD is True) and \
        max(bounds[i + 1] - bounds[i] for i in range(len(bounds) - 1)) <= int(getattr(rm.config, "max_chunk_frames", 32))
    for i in range(len(bounds) - 1):                                                      # :534-537
        if ahead and i + 2 < len(bounds):
            rm.project_ahead(x[bounds[i + 1]:bounds[i + 2]])
        rm(x[bounds[i]:bounds[i + 1]])
    if rm._cache_mode == "autograd" or _tail_wants_grad(model, memory_prompt_embeds, frame_prompt_embeds, image_newline):
        # training.  With `recurrent_memory_transformer` frozen but a trainable fuser / token-type embedding / newline /
        # prompt embedding (mm_tunable_parts="larimar_model", train.py:1708-1713) the chunks above ran on the engine
        # (nothing to differentiate there) and only the tail below records a graph - on CLONES of the ring views, which
        # the next video would overwrite before backward.
        return _video_memory_tokens_autograd(model, rm, x, fine_cpu, memory_prompt_embeds, frame_prompt_embeds,
                                             image_newline, with_frames, out, layout)
    eng = rm.engine(image.device, image.dtype)
    n = len(rm.memory_cache)
    R = rm.num_memory_tokens * P
    n_fine = fine_cpu.numel()
    mem_rows = layout_block_rows(n * R, layout, P)
    rows = memory_prompt_embeds.shape[0] + mem_rows
    if with_frames:
        rows += frame_prompt_embeds.shape[0] + layout_block_rows(n_fine * P, layout, P)
    if out is None:
        out = torch.empty((rows, D), device=image.device, dtype=image.dtype)
    elif tuple(out.shape) != (rows, D) or out.dtype != image.dtype or not out.is_contiguous() or not out.is_cuda:
        raise capi.MavlmError(f"video_memory_tokens: `out` must be a contiguous [{rows},{D}] {image.dtype} GPU tensor")
    mp = memory_prompt_embeds.to(image.dtype).contiguous()
    fp = frame_prompt_embeds.to(image.dtype).contiguous()
    nl, nl_ptr = _newline_ptr(image_newline, layout, image.device, image.dtype)
    written = ctypes.c_int64(0)
    capi.check(capi.lib().mavlm_fuse_emit_layout(eng.ctx, x.data_ptr(), _device_indices(fine_cpu, image.device).data_ptr(), n_fine,
                                                 mp.data_ptr(), mp.shape[0], fp.data_ptr(), fp.shape[0], nl_ptr,
                                                 1 if with_frames else 0, capi.LAYOUTS[layout], out.data_ptr(), rows,
                                                 ctypes.byref(written), ops.stream_ptr()), "mavlm_fuse_emit_layout")
    assert written.value == rows
    return out, {"num_memories": n, "pe_frames": x, "fine_idx": fine_cpu, "memory_rows": _memory_rows(mp.shape[0], n, R, layout, P)}


def _memory_rows(mp_rows, n, R, layout, P):
    """`info["memory_rows"]`: the rows of the memory block inside a token block - with the newlines INSIDE it ("frame" / "grid"),
    without the one behind it ("one_token")"""
    return mp_rows, mp_rows + (layout_block_rows(n * R, layout, P) if layout_period(layout, P) else n * R)


def _prepare_row_batch(kind, name, model, bp, images, frame_idx_cpu, chunk, fine_frames, emit=True):
    """What every row-batch driver does before the first step.  `kind`: "equal" (bp.batch videos of one length), "ragged"
    (2 .. bp.batch videos, each a positive multiple of `chunk` frames, the same number of fine frames) or "clips" (2 .. bp.batch
    videos of 1 .. chunk - 1 frames); `name`: the public function the caller called, for the error texts.  Validates the images
    (GPU, [T_b, P, D], one dtype and device, the length rule of the kind) and `frame_idx_cpu` (one index tensor per video, of its
    length; for "equal" also one tensor shared by all: two videos of 130 and 150 input frames both sample 128 frames, at other
    original indices), orders the videos longest first (stable: the caller's order for equal lengths), adds the positional
    encoding per video (llava_arch.py:510-511; consecutive videos with the same index tensor share its check and device copy)
    and computes the fine-frame indices (:513-522).  Returns (xs, fines, order, back) - PE-added frames and fine indices in the
    stepping order, `order[j]` = the caller's position of the j-th video stepped, `back` its inverse.  `emit` False: the caller
    builds the blocks from torch ops and the plain GEMMs (the training tail), so the hidden-size rule of the clip emit does not
    apply."""
    k = len(images)
    if (k != bp.batch) if kind == "equal" else (not 2 <= k <= bp.batch):
        raise capi.MavlmError(f"{name}: {bp.batch if kind == 'equal' else f'2..{bp.batch}'} videos expected")
    P, D = images[0].shape[1:]
    dev, dt = images[0].device, images[0].dtype
    for im in images:
        if not im.is_cuda or im.dim() != 3 or tuple(im.shape[1:]) != (P, D) or im.dtype != dt or im.device != dev:
            raise capi.MavlmError(f"{name}: GPU frame tokens [T_b, P, D] of one dtype / device expected")
        T = im.shape[0]
        if kind == "equal" and T != images[0].shape[0]:
            raise capi.MavlmError(f"{name}: GPU frame tokens of one shape / dtype expected (videos of different lengths: "
                                  "`ragged=True`, `video_memory_tokens_clips`, `video_memory_tokens_ragged_train`)")
        if kind == "ragged" and (T < chunk or T % chunk):
            raise capi.MavlmError(f"{name}: every video length must be a positive multiple of the chunk ({chunk} frames); got {T}")
        if kind == "clips" and not 1 <= T < chunk:
            raise capi.MavlmError(f"{name}: a clip has 1..{chunk - 1} frames (one chunk of all its frames); got {T}")
    if isinstance(frame_idx_cpu, (list, tuple)):
        idxs = list(frame_idx_cpu)
    else:
        idxs = [frame_idx_cpu] * k if kind == "equal" else []
    if len(idxs) != k or any(i.numel() != im.shape[0] for i, im in zip(idxs, images)):
        raise capi.MavlmError(f"{name}: one frame index tensor per video, of its length")
    if kind == "clips" and emit and D % 256:         # (refused before any step: mavlm_fuse_emit_layout_frames_to would, afterwards)
        raise capi.MavlmError(f"{name}: the clip emit needs a hidden size that is a multiple of 256; got {D}")
    pe: TemporalPositionalEncoding = model.positional_encoding
    order = sorted(range(k), key=lambda i: -images[i].shape[0])            # longest first; stable in the caller's order
    back = [0] * k                                   # caller's position -> position in the stepping order
    for j, i in enumerate(order):
        back[i] = j
    xs, fines, fine_of, last, last_dev = [], [], {}, None, None
    for i in order:
        if idxs[i] is not last:
            pe.check_indices(idxs[i])
            last, last_dev = idxs[i], _device_indices(idxs[i], dev)
        xs.append(pe(images[i], last_dev, indices_checked=True))                                    # :510-511
        T = images[i].shape[0]
        if T not in fine_of:
            fine_of[T] = fine_frame_indices(T, fine_frames)                                         # :513-522
        fines.append(fine_of[T])
    if kind == "ragged" and any(f.numel() != fines[0].numel() for f in fines):
        raise capi.MavlmError(f"{name}: the videos must have the same number of fine frames")
    return xs, fines, order, back


def _step_chunks(step, xs, chunk, ragged):
    """Hands the videos' chunks (llava_arch.py:528,534-537) to `step` (`bp.step` / `bp.step_train`).  Equal lengths: every video's
    chunk i, the last one shorter where the length is no multiple of `chunk`.  `ragged` (`xs` longest first, lengths multiples
    of `chunk`): step i takes chunk i of the videos that still have one - a prefix that only shrinks."""
    if ragged:
        chunks = [x.shape[0] // chunk for x in xs]
        for i in range(chunks[0]):
            step([x[i * chunk:(i + 1) * chunk] for x, c in zip(xs, chunks) if c > i])
        return
    bounds = uniform_segment_variant(xs[0].shape[0], chunk)
    for i in range(len(bounds) - 1):
        step([x[bounds[i]:bounds[i + 1]] for x in xs])


def _block_destination(name, out, dst_rows, rows, order, stacked, D, dev, dt):
    """Where the emit writes the blocks (`rows[j]` rows for the j-th video stepped).  Returns (buffer, dst): with `dst_rows` the
    caller's contiguous [out_rows, D] `out` and each video's first row in it; without, for `stacked` blocks (equal lengths) a
    [k, rows, D] tensor - the caller's `out` or a new one - and None (constant stride), else ONE new [sum(rows), D] buffer and
    the running offsets."""
    k = len(rows)
    if dst_rows is not None:
        if out is None or out.dim() != 2 or out.shape[1] != D or out.dtype != dt or not out.is_contiguous() or not out.is_cuda \
                or len(dst_rows) != k:
            raise capi.MavlmError(f"{name}: `dst_rows` needs {k} rows of a contiguous [out_rows,{D}] {dt} GPU tensor `out`")
        return out, [int(dst_rows[i]) for i in order]
    if stacked:
        if out is None:
            out = torch.empty((k, rows[0], D), device=dev, dtype=dt)
        elif tuple(out.shape) != (k, rows[0], D) or out.dtype != dt or not out.is_contiguous() or not out.is_cuda:
            raise capi.MavlmError(f"{name}: `out` must be a contiguous [{k},{rows[0]},{D}] {dt} GPU tensor")
        return out, None
    if out is not None:
        raise capi.MavlmError(f"{name}: `out` goes with `dst_rows` (the blocks differ in length)")
    return torch.empty((sum(rows), D), device=dev, dtype=dt), [sum(rows[:j]) for j in range(k)]


def _emit_row_batch(kind, eng, xs, fines, mp, fp, nl_ptr, with_frames, layout, buf, dst, rows):
    """ONE emit for the blocks of every video of a row batch (fuser MLP + type adds + prompts / newlines, written in place).  The
    export follows the kind of the batch and the destination - the equal-length and the ragged implementation group the fuser
    GEMMs differently, so the choice is part of the result: mavlm_fuse_emit_layout_batch (equal lengths, stacked blocks) /
    _batch_to (equal lengths, `dst`) / _ragged_to (per ring slot the fuser runs over the videos that hold it; a fine-frame
    index row per video) / _frames_to (clips: a fine-frame count per video)."""
    lib, k, dev = capi.lib(), len(xs), xs[0].device
    xptrs = (capi.vp * k)(*[x.data_ptr() for x in xs])
    tail = (mp.data_ptr(), mp.shape[0], fp.data_ptr(), fp.shape[0], nl_ptr, 1 if with_frames else 0, capi.LAYOUTS[layout])
    if kind == "equal":
        written = ctypes.c_int64(0)
        fine = (_device_indices(fines[0], dev).data_ptr(), fines[0].numel())
        if dst is None:
            capi.check(lib.mavlm_fuse_emit_layout_batch(eng.ctx, xptrs, *fine, *tail, buf.data_ptr(), rows[0], ctypes.byref(written),
                                                        ops.stream_ptr()), "mavlm_fuse_emit_layout_batch")
        else:
            capi.check(lib.mavlm_fuse_emit_layout_batch_to(eng.ctx, xptrs, *fine, *tail, buf.data_ptr(), buf.shape[0],
                                                           (ctypes.c_int64 * k)(*dst), ctypes.byref(written), ops.stream_ptr()),
                       "mavlm_fuse_emit_layout_batch_to")
        assert written.value == rows[0]
        return
    written = (ctypes.c_int64 * k)()
    where = (buf.data_ptr(), buf.shape[0], (ctypes.c_int64 * k)(*dst), written, ops.stream_ptr())
    if kind == "ragged":
        fine_dev = _device_indices(torch.cat(fines), dev)                        # [k, n_fine], one row per video
        capi.check(lib.mavlm_fuse_emit_layout_ragged_to(eng.ctx, k, xptrs, fine_dev.data_ptr(), fines[0].numel(), *tail, *where),
                   "mavlm_fuse_emit_layout_ragged_to")
    else:
        n_fines = [int(f.numel()) for f in fines]
        fine_ld = max(n_fines) + (max(n_fines) & 1)                              # (even: every index row starts 16-byte aligned)
        fine_cpu = torch.zeros((k, fine_ld), dtype=torch.long)
        for j, f in enumerate(fines):
            fine_cpu[j, :f.numel()] = f
        fine_dev = _device_indices(fine_cpu.reshape(-1), dev)                    # [k, fine_ld], one row per video
        capi.check(lib.mavlm_fuse_emit_layout_frames_to(eng.ctx, k, xptrs, fine_dev.data_ptr(), fine_ld, (capi.i32 * k)(*n_fines),
                                                        *tail, *where), "mavlm_fuse_emit_layout_frames_to")
    assert list(written) == rows


def _row_batch_info(kind, bp, xs, fines, counts, rows, order, back, mp_rows, layout):
    """`info` of a row-batch call.  "equal": one `num_memories`, `fine_idx`, `block_rows` for all videos and `memory_rows`;
    otherwise `order` and per-video lists in the caller's order.  `counts`, `rows`: memories and block rows per video in the
    stepping order (`rows` None: no `block_rows`)."""
    if kind == "equal":
        P = xs[0].shape[1]
        info = {"num_memories": counts[0], "pe_frames": xs, "fine_idx": fines[0], "frame_scores": bp.frame_scores,
                "memory_rows": _memory_rows(mp_rows, counts[0], bp.proj.num_memory_tokens * P, layout, P)}
    else:
        info = {"order": order, "num_memories": [counts[j] for j in back], "pe_frames": [xs[j] for j in back],
                "fine_idx": [fines[j] for j in back], "frame_scores": bp.frame_scores}
    if rows is not None:
        info["block_rows"] = rows[0] if kind == "equal" else [rows[j] for j in back]
    return info


def _row_batch_tokens(kind, name, model, bp, images, frame_idx_cpu, memory_prompt_embeds, frame_prompt_embeds, image_newline,
                      with_frames, chunk, fine_frames, out, layout, dst_rows):
    """The inference driver of every row batch (`kind`, `name`: see _prepare_row_batch): prepare, `bp.reset()`, the steps, the
    destination, one emit, `info`."""
    layout_period(layout, images[0].shape[1])
    xs, fines, order, back = _prepare_row_batch(kind, name, model, bp, images, frame_idx_cpu, chunk, fine_frames)
    bp.reset()                                                                             # :532
    if kind == "clips":
        bp.step_frames(xs)                                                                 # :534-537: one chunk each
    else:
        _step_chunks(bp.step, xs, chunk, kind == "ragged")                                 # :534-537
    P, D = xs[0].shape[1:]
    dev, dt = xs[0].device, xs[0].dtype
    eng = bp.engine(dev, dt)
    M, cap, mp_rows = bp.proj.num_memory_tokens, eng.c.cache_cap, memory_prompt_embeds.shape[0]
    rows = [video_token_rows(x.shape[0], M, P, with_frames, chunk, fine_frames, cap, mp_rows, frame_prompt_embeds.shape[0], layout)
            for x in xs]
    buf, dst = _block_destination(name, out, dst_rows, rows, order, kind == "equal", D, dev, dt)
    mp = memory_prompt_embeds.to(dt).contiguous()
    fp = frame_prompt_embeds.to(dt).contiguous()
    nl, nl_ptr = _newline_ptr(image_newline, layout, dev, dt)
    _emit_row_batch(kind, eng, xs, fines, mp, fp, nl_ptr, with_frames, layout, buf, dst, rows)
    info = _row_batch_info(kind, bp, xs, fines, [min(-(-x.shape[0] // chunk), cap) for x in xs], rows, order, back, mp_rows, layout)
    if kind == "equal" or dst_rows is not None:
        return buf, info
    return [buf[dst[j]:dst[j] + rows[j]] for j in back], info


@torch.no_grad()
def video_memory_tokens_batched(model, bp: BatchedProjector, images, frame_idx_cpu,
                                memory_prompt_embeds: torch.Tensor, frame_prompt_embeds: torch.Tensor,
                                image_newline: Optional[torch.Tensor], with_frames: bool = True, chunk: int = 32,
                                fine_frames: int = 32, out: Optional[torch.Tensor] = None, layout: str = "one_token",
                                dst_rows: Optional[List[int]] = None, ragged: bool = False):
    """`video_memory_tokens` for B videos of the SAME length stepped together (row batch, `BatchedProjector`): every
    weight-shared GEMM / LayerNorm of the path runs once over the stacked memory rows of all videos.  `images`: B tensors
    [T,196,D]; `frame_idx_cpu`: the original frame indices (shared: same length, same sampling).  Returns
    (tokens [B, rows, D] - video b's block is tokens[b] -, info).  Inference only.  `layout`: as video_memory_tokens.
    `frame_idx_cpu` may be a list of B index tensors of one length.
    `dst_rows` (with `out` = a contiguous [out_rows, D] buffer, e.g. the padded inputs_embeds of a batch of samples seen as
    rows): video b's block is written at row dst_rows[b] of `out` (mavlm_fuse_emit_layout_batch_to: the same launches, one
    destination per video; rows outside the blocks are not touched); returns (out, info) with info["block_rows"].
    `ragged=True`: k videos (2 <= k <= B) of T_b = c_b * `chunk` frames - lengths that may differ - on the one engine.  Internally
    the videos are ordered by chunk count, longest first (stable); step i takes chunk i of the videos that still have one - a
    prefix that only shrinks (`BatchedProjector.step`) -; ONE emit at the end writes every video's block
    (`mavlm_fuse_emit_layout_ragged_to`).  `frame_idx_cpu`: one index tensor per video.  Returns (list of [rows_b, D] blocks in
    the caller's order - or `out` with `dst_rows` -, info with `order` and per-video lists).  Without it unequal shapes are
    refused."""
    return _row_batch_tokens("ragged" if ragged else "equal",
                             "video_memory_tokens_batched(ragged=True)" if ragged else "video_memory_tokens_batched", model, bp,
                             images, frame_idx_cpu, memory_prompt_embeds, frame_prompt_embeds, image_newline, with_frames, chunk,
                             fine_frames, out, layout, dst_rows)


@torch.no_grad()
def video_memory_tokens_clips(model, bp: BatchedProjector, images, frame_idx_cpu, memory_prompt_embeds: torch.Tensor,
                              frame_prompt_embeds: torch.Tensor, image_newline: Optional[torch.Tensor], with_frames: bool = True,
                              chunk: int = 32, fine_frames: int = 32, out: Optional[torch.Tensor] = None,
                              layout: str = "one_token", dst_rows: Optional[List[int]] = None):
    """`video_memory_tokens` for k clips (2 <= k <= bp.batch) of 1 <= T_b < `chunk` frames each on one row-batched engine: every
    clip is ONE chunk of all its frames (llava_arch.py:528), so the k videos take one step together - different frame counts
    in one step (`BatchedProjector.step_frames`) - and one emit with a fine-frame count per video
    (`mavlm_fuse_emit_layout_frames_to`; a clip's fine frames are all its frames, :513-522).  Internally the clips are ordered
    longest first (stable).  `images`: k tensors [T_b, P, D]; `frame_idx_cpu`: one index tensor per clip.  Returns (list of
    [rows_b, D] blocks in the caller's order - or `out`, a contiguous [out_rows, D] buffer, with `dst_rows` -, info).  Inference."""
    return _row_batch_tokens("clips", "video_memory_tokens_clips", model, bp, images, frame_idx_cpu, memory_prompt_embeds,
                             frame_prompt_embeds, image_newline, with_frames, chunk, fine_frames, out, layout, dst_rows)


def video_memory_tokens_batched_train(model, bp: BatchedProjector, images, frame_idx_cpu,
                                      memory_prompt_embeds: torch.Tensor, frame_prompt_embeds: torch.Tensor,
                                      image_newline: Optional[torch.Tensor], with_frames: bool = True, chunk: int = 32,
                                      fine_frames: int = 32, layout: str = "one_token"):
    """`video_memory_tokens_batched` under autograd: B videos of the same length stepped together by
    `BatchedProjector.step_train`, then the tail of the single-video training path (`_train_block`) for every video - the fuser
    MLP runs ONCE over the B * n * M * 196 stacked memory rows (HIP autograd Functions); the token-type adds, the layout and the
    concatenation are torch ops, so autograd routes the gradients of token_type_embedding, the prompt embeddings and
    image_newline as in the reference.  Returns (tokens [B, rows, D] with grad - the bits of `video_memory_tokens_batched` -,
    info).  `frame_idx_cpu`: shared, or a list of one index tensor per video.  Videos of different lengths:
    `video_memory_tokens_ragged_train`."""
    from .. import _autograd as ag
    layout_period(layout, images[0].shape[1])
    xs, fines, order, back = _prepare_row_batch("equal", "video_memory_tokens_batched_train", model, bp, images, frame_idx_cpu,
                                                chunk, fine_frames)
    bp.reset()                                                                             # :532
    _step_chunks(bp.step_train, xs, chunk, False)                                          # :534-537
    B, n = bp.batch, len(bp._tcache)
    P, D = xs[0].shape[1:]
    R = bp.proj.num_memory_tokens * P
    mem = torch.cat(bp._tcache, dim=0)                                                     # [n * B * R, D], oldest first (:545)
    fused = ag.fuser_mlp(model.memory_fuser, mem, model.token_type_embedding.weight[0], fused_gelu=True).view(n, B, R, D)   # :546-553
    nl, mp, fp = _train_tail_operands(image_newline, memory_prompt_embeds, frame_prompt_embeds, layout, xs[0])
    toks = [_train_block(model, fused[:, b].reshape(n * R, D), xs[b], fines[b], mp, fp, nl, with_frames, layout) for b in range(B)]
    return torch.stack(toks), _row_batch_info("equal", bp, xs, fines, [n] * B, None, order, back, mp.shape[0], layout)


def video_memory_tokens_clips_train(model, bp: BatchedProjector, images, frame_idx_cpu, memory_prompt_embeds: torch.Tensor,
                                    frame_prompt_embeds: torch.Tensor, image_newline: Optional[torch.Tensor],
                                    with_frames: bool = True, chunk: int = 32, fine_frames: int = 32, layout: str = "one_token"):
    """`video_memory_tokens_clips` under autograd: k clips (2 <= k <= bp.batch) of 1 <= T_b < `chunk` frames each, ordered
    longest first (stable), take ONE step together - `BatchedProjector.step_train_frames`: the variable-length attention forward
    and backward over the packed chunk K/V - then the fuser runs over the k * R stacked memory rows in one GEMM pair and
    `_train_block` builds every video's block (every frame of a clip is a fine frame).  Where that GEMM pair does not split its
    contraction the feature rows are the bits of the inference clip block.  The block is built from torch ops and the plain
    GEMMs: every hidden size the training path takes, 896 included (the inference clip emit needs a multiple of 256).  Heads of
    448 columns: clips of different lengths are refused (`step_train_frames`) unless `ops.set_attention_hd_varlen_train(True)`
    (off by default) - with it the step runs the variable-length 448 forward and backward.  Returns (list of [rows_b, D] blocks with grad in the caller's order, info as
    `video_memory_tokens_clips`)."""
    from .. import _autograd as ag
    layout_period(layout, images[0].shape[1])
    xs, fines, order, back = _prepare_row_batch("clips", "video_memory_tokens_clips_train", model, bp, images, frame_idx_cpu, chunk,
                                                fine_frames, emit=False)
    k = len(xs)
    bp.reset()                                                                             # :532
    bp.step_train_frames(xs)                                                               # :534-537: one chunk each
    P, D = xs[0].shape[1:]
    R = bp.proj.num_memory_tokens * P
    fused = ag.fuser_mlp(model.memory_fuser, bp._tcache[-1], model.token_type_embedding.weight[0], fused_gelu=True)   # :545-553
    nl, mp, fp = _train_tail_operands(image_newline, memory_prompt_embeds, frame_prompt_embeds, layout, xs[0])
    toks = [_train_block(model, fused[b * R:(b + 1) * R], xs[b], fines[b], mp, fp, nl, with_frames, layout) for b in range(k)]
    info = _row_batch_info("clips", bp, xs, fines, [1] * k, [t.shape[0] for t in toks], order, back, mp.shape[0], layout)
    return [toks[j] for j in back], info


def _ragged_fuser_rows(lib, counts, R, D, inter):
    """Does the fuser's GEMM pair give the same bits over ALL stacked FIFO rows as over the rows of the videos that hold one
    ring slot (the grouping of `mavlm_fuse_emit_layout_ragged_to`)?  The kernels are row-independent; only a split contraction -
    `mavlm_linear_ws_floats`, a function of the row count - sums in another order.  `counts`: memories per video, longest first."""
    rows = {sum(counts) * R} | {sum(1 for c in counts if c > sl) * R for sl in range(max(counts))}
    return all(lib.mavlm_linear_ws_floats(m, inter, D, capi.EPI_GELU, inter) == 0 and
               lib.mavlm_linear_ws_floats(m, D, inter, capi.EPI_BIAS, D) == 0 for m in rows)


def video_memory_tokens_ragged_train(model, bp: BatchedProjector, images, frame_idx_cpu, memory_prompt_embeds: torch.Tensor,
                                     frame_prompt_embeds: torch.Tensor, image_newline: Optional[torch.Tensor],
                                     with_frames: bool = True, chunk: int = 32, fine_frames: int = 32, layout: str = "one_token"):
    """`video_memory_tokens_batched(ragged=True)` under autograd - the ragged form of `video_memory_tokens_batched_train`: 2 .. B
    videos whose lengths are positive multiples of `chunk` and may differ, one frame index tensor each, the same number of fine
    frames.  The videos are ordered longest first (stable) and stepped by `BatchedProjector.step_train(ragged=True)`; the fuser
    runs over all videos' FIFO rows in one stacked GEMM pair where no row count involved splits its contraction, else in one
    pair per ring slot over the videos that hold it - either way the feature rows are the ragged inference block's bits.  Type
    rows, layout and concatenation are torch ops, as on the equal-length path.  Returns (list of [rows_b, D] blocks with grad
    in the caller's order, the info of the ragged inference call: `order`, per-video `num_memories`, `block_rows`, ...)."""
    from .. import _autograd as ag
    layout_period(layout, images[0].shape[1])
    xs, fines, order, back = _prepare_row_batch("ragged", "video_memory_tokens_ragged_train", model, bp, images, frame_idx_cpu,
                                                chunk, fine_frames)
    k = len(xs)
    chunks = [x.shape[0] // chunk for x in xs]
    bp.reset()                                                                                      # :532
    _step_chunks(lambda segs: bp.step_train(segs, ragged=True), xs, chunk, True)                    # :534-537, per video
    caches = [bp.memory_cache(b) for b in range(k)]                          # per video, oldest first
    counts = [len(c) for c in caches]
    P, D = xs[0].shape[1:]
    rm: TransformerProjector = model.recurrent_memory_transformer
    R = rm.num_memory_tokens * P
    temb = model.token_type_embedding.weight
    fuser = model.memory_fuser
    if _ragged_fuser_rows(capi.lib(), counts, R, D, fuser[0].weight.shape[0]):
        mem = torch.cat([m.reshape(R, D) for c in caches for m in c], dim=0)                        # :545, every video
        fused = ag.fuser_mlp(fuser, mem, temb[0], fused_gelu=True)                                  # :546-553
        at = [sum(counts[:b]) * R for b in range(k + 1)]
        blocks = [fused[at[b]:at[b + 1]] for b in range(k)]
    else:
        # per ring slot (memory g of a video lives in slot g % cap), over the videos 0 .. h-1 that hold it
        cap = int(getattr(rm.config, "cache_cap", 10))
        place = [[None] * n for n in counts]
        for sl in range(max(counts)):
            hold = [b for b in range(k) if counts[b] > sl]
            pos = [sl if chunks[b] <= cap else (sl - chunks[b] % cap + cap) % cap for b in hold]
            out_sl = ag.fuser_mlp(fuser, torch.cat([caches[b][p].reshape(R, D) for b, p in zip(hold, pos)], dim=0), temb[0],
                                  fused_gelu=True)
            for j, (b, p) in enumerate(zip(hold, pos)):
                place[b][p] = out_sl[j * R:(j + 1) * R]
        blocks = [torch.cat(pl, dim=0) for pl in place]
    nl, mp, fp = _train_tail_operands(image_newline, memory_prompt_embeds, frame_prompt_embeds, layout, xs[0])
    toks = [_train_block(model, blocks[b], xs[b], fines[b], mp, fp, nl, with_frames, layout) for b in range(k)]
    info = _row_batch_info("ragged", bp, xs, fines, counts, [t.shape[0] for t in toks], order, back, mp.shape[0], layout)
    return [toks[j] for j in back], info


ROW_BATCH_SIZES = (8, 4, 2)


def plan_row_batches(keys, sizes=ROW_BATCH_SIZES):
    """Which videos of a forward step together.  `keys`: one hashable per video, in input order (the sampled frame count, with
    whatever else has to agree inside a row batch); videos with equal keys form a group, consecutive or not.  A group is cut
    into row batches of the sizes in `sizes`, largest first; what is left of it runs as single videos.  Returns
    (batches, singles): lists of input positions (a batch in input order, the batches in the order of their first video), and
    the positions of the singles, ascending.  Three sizes bound the number of batched engines a model keeps; the batched emit
    takes at most 16 videos per launch."""
    sizes = sorted({int(s) for s in sizes}, reverse=True)
    if any(s < 2 or s > 16 for s in sizes):
        raise ValueError("row batch sizes: 2 .. 16 videos")
    groups = {}
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    batches, singles = [], []
    for members in groups.values():
        at = 0
        for s in sizes:
            while len(members) - at >= s:
                batches.append(members[at:at + s])
                at += s
        singles += members[at:]
    batches.sort(key=lambda b: b[0])
    return batches, sorted(singles)


RAGGED_MAX_GROUP = 8


def plan_ragged_batches(lengths, chunk=32, keys=None, sizes=ROW_BATCH_SIZES):
    """Which videos of a forward step together when a row batch may hold videos of different lengths (ragged row batches).
    `lengths`: the sampled frame count of each video, in input order; a video is eligible when its length is a positive multiple
    of `chunk` - its chunk count is length / chunk.  `keys`: one hashable per video with what else has to agree inside a batch
    (dtype, device) - default: nothing.
    Eligible videos with one key are sorted by chunk count, longest first, stable in input order.  A video joins the current
    group while the group has fewer than 8 videos and its chunk count is at least HALF that of the group's longest video;
    otherwise it opens a new group.  A group of k >= 2 videos runs on ONE row-batched engine: the smallest size in `sizes`
    that is >= k (3 -> 4, 5 / 6 / 7 -> 8), stepped as a shrinking prefix.  Groups of one and the videos that are not eligible
    go where they go today: through `plan_row_batches` over (length, key).
    The "half" bound limits the stretch a lone survivor runs on the row-batch schedule at one video; it is a policy picked
    WITHOUT a measurement (tools/diag_ragged_batch.py reports what a lopsided pair costs).
    Returns (ragged, batches, singles): `ragged` = [(engine size, positions longest first)], the groups in the order of their
    first (longest) video; `batches`, `singles` = as `plan_row_batches` returns them, for the rest."""
    sizes_up = sorted({int(s) for s in sizes})
    if any(s < 2 or s > 16 for s in sizes_up):
        raise ValueError("row batch sizes: 2 .. 16 videos")
    n = len(lengths)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("plan_ragged_batches: chunk >= 1")
    chunk_counts = [int(t) // chunk if int(t) > 0 and int(t) % chunk == 0 else 0 for t in lengths]
    keys = [None] * n if keys is None else list(keys)
    if len(keys) != n:
        raise ValueError("plan_ragged_batches: one key per video")
    cap = min(RAGGED_MAX_GROUP, sizes_up[-1]) if sizes_up else 0
    by_key = {}
    for i, c in enumerate(chunk_counts):
        if c > 0:
            by_key.setdefault(keys[i], []).append(i)
    ragged, taken = [], set()
    for members in by_key.values():
        members = sorted(members, key=lambda i: -int(chunk_counts[i]))       # (stable: input order among equal counts)
        groups, cur = [], []
        for i in members:
            if cur and len(cur) < cap and 2 * int(chunk_counts[i]) >= int(chunk_counts[cur[0]]):
                cur.append(i)
            else:
                if cur:
                    groups.append(cur)
                cur = [i]
        if cur:
            groups.append(cur)
        for g in groups:
            if len(g) >= 2:
                ragged.append((next(s for s in sizes_up if s >= len(g)), g))
                taken.update(g)
    ragged.sort(key=lambda sg: min(sg[1]))
    rest = [i for i in range(n) if i not in taken]
    batches, singles = plan_row_batches([(int(lengths[i]), keys[i]) for i in rest], sizes)
    return ragged, [[rest[j] for j in b] for b in batches], [rest[j] for j in singles]


CLIP_MAX_FRAMES = 32        # a video of fewer frames is ONE chunk of all its frames (sample_frame_count, uniform_segment_variant)


def plan_clip_batches(lengths, keys=None, sizes=ROW_BATCH_SIZES):
    """Which CLIPS of a forward step together (clip row batches: different frame counts in one step).
    `lengths`: the sampled frame count of each video, in input order; a video is eligible when 0 < length < 32 - it then runs
    as one chunk of all its frames, and no two such videos of different lengths share a row batch otherwise.  Equal lengths
    are eligible too (their group takes the equal-F step).  `keys`: as in `plan_ragged_batches`.
    Eligible videos with one key are sorted by length, longest first, stable in input order.  A video joins the current group
    while the group has fewer than 8 videos and its length is at least HALF that of the group's longest video; otherwise it
    opens a new group.  A group of k >= 2 videos runs on ONE row-batched engine: the smallest size in `sizes` that is >= k.
    The "half" bound keeps the key counts of a variable-length launch within a factor of two (the longest video's workgroups
    set its duration); like the bound of `plan_ragged_batches` it is a policy picked WITHOUT a measurement
    (tools/diag_clip_batch.py times one group).
    Returns (clips, rest): `clips` = [(engine size, positions longest first)], the groups in the order of their first video;
    `rest` = the positions of every other video, ascending - they go through today's planners."""
    sizes_up = sorted({int(s) for s in sizes})
    if any(s < 2 or s > 16 for s in sizes_up):
        raise ValueError("row batch sizes: 2 .. 16 videos")
    n = len(lengths)
    keys = [None] * n if keys is None else list(keys)
    if len(keys) != n:
        raise ValueError("plan_clip_batches: one key per video")
    cap = min(RAGGED_MAX_GROUP, sizes_up[-1]) if sizes_up else 0
    by_key = {}
    for i, t in enumerate(lengths):
        if 0 < int(t) < CLIP_MAX_FRAMES:
            by_key.setdefault(keys[i], []).append(i)
    clips, taken = [], set()
    for members in by_key.values():
        members = sorted(members, key=lambda i: -int(lengths[i]))            # (stable: input order among equal lengths)
        groups, cur = [], []
        for i in members:
            if cur and len(cur) < cap and 2 * int(lengths[i]) >= int(lengths[cur[0]]):
                cur.append(i)
            else:
                if cur:
                    groups.append(cur)
                cur = [i]
        if cur:
            groups.append(cur)
        for g in groups:
            if len(g) >= 2:
                clips.append((next(s for s in sizes_up if s >= len(g)), g))
                taken.update(g)
    clips.sort(key=lambda sg: min(sg[1]))
    return clips, [i for i in range(n) if i not in taken]


class VideoPlacement:
    """Where everything of a batch of samples lands in the padded [B, Lmax, D] `inputs_embeds` buffer when each video block is
    emitted in place - what `splice_into_text` arrives at by concatenating and padding, computed on the host from the token ids
    alone.  Fields:
      general     True: a sample is longer than tokenizer_model_max_length (the cut may fall into a block): take the general
                  path (`splice_into_text`); only `lengths` and `Lmax` (after the cut) are filled in then
      Lmax        padded length;  lengths[s]: rows of sample s;  starts[s]: its first row (left padding: Lmax - lengths[s])
      video_of[s] the video of sample s (-1: text only);  image_at[s]: position of its image token among its ids (-1)
      dst_row[v]  first row of video v's block in the buffer seen as [B * Lmax, D]
      segments    (sample, first id, end id, first row inside the sample's Lmax rows): runs of text ids -> rows
      padding     (sample, first row, end row): rows left zero
    """

    def __init__(self, ids_list, block_rows, left=False, max_tok=None):
        ids_list = [i.tolist() if torch.is_tensor(i) else list(i) for i in ids_list]
        self.block_rows = [int(r) for r in block_rows]
        self.video_of, self.image_at, self.lengths = [], [], []
        v = 0
        for ids in ids_list:
            at = [i for i, t in enumerate(ids) if t == IMAGE_TOKEN_INDEX]
            if len(at) > 1 or (at and v >= len(block_rows)):
                raise NotImplementedError(_ONE_VIDEO_PER_SAMPLE)
            self.video_of.append(v if at else -1)
            self.image_at.append(at[0] if at else -1)
            self.lengths.append(len(ids) - 1 + int(block_rows[v]) if at else len(ids))
            v += len(at)
        if v != len(block_rows):
            raise NotImplementedError(_ONE_VIDEO_PER_SAMPLE)
        self.general = max_tok is not None and any(n > max_tok for n in self.lengths)
        if self.general:
            self.lengths = [min(n, max_tok) for n in self.lengths]
        self.left = bool(left)
        self.Lmax = L = max(self.lengths)
        self.starts = [L - n if self.left else 0 for n in self.lengths]
        self.dst_row, self.segments, self.padding = [0] * len(block_rows), [], []
        if self.general:
            return
        for s, ids in enumerate(ids_list):
            st, n, p = self.starts[s], self.lengths[s], self.image_at[s]
            if n < L:
                self.padding.append((s, 0, st) if self.left else (s, n, L))
            if p < 0:
                if n:
                    self.segments.append((s, 0, n, st))
                continue
            rows = int(block_rows[self.video_of[s]])
            self.dst_row[self.video_of[s]] = s * L + st + p
            if p:
                self.segments.append((s, 0, p, st))
            if p + 1 < len(ids):
                self.segments.append((s, p + 1, len(ids), st + p + rows))

    def labels_mask_positions(self, lab_list, attention_mask, position_ids):
        """(labels [B, Lmax] or None when `lab_list` is None, attention mask or None, position ids or None) as `splice_into_text`
        builds them (llava_arch.py:745-878): IGNORE_INDEX over every block and the padding, mask True and positions 0..n-1 over
        a sample's rows, zeros in the padding.  `lab_list`: the labels of each sample's ids (padding removed)."""
        B, L = len(self.lengths), self.Lmax
        labels = mask = pos = None
        if lab_list is not None:
            labels = torch.full((B, L), IGNORE_INDEX, dtype=lab_list[0].dtype, device=lab_list[0].device)
            for s, lo, hi, row in self.segments:
                labels[s, row:row + hi - lo] = lab_list[s][lo:hi]
        if attention_mask is not None:
            mask = torch.zeros((B, L), dtype=torch.bool, device=attention_mask.device)
            for s, (st, n) in enumerate(zip(self.starts, self.lengths)):
                mask[s, st:st + n] = True
            mask = mask.to(dtype=attention_mask.dtype)
        if position_ids is not None:
            pos = torch.zeros((B, L), dtype=position_ids.dtype, device=position_ids.device)
            for s, (st, n) in enumerate(zip(self.starts, self.lengths)):
                pos[s, st:st + n] = torch.arange(0, n, dtype=pos.dtype, device=pos.device)
        return labels, mask, pos


_ONE_VIDEO_PER_SAMPLE = ("the memory path supports one video per sample: with several videos in a forward, exactly as many samples "
                         "as videos hold an image token, one each (llava_arch.py:436: 'Now support only batch size of 1'; a second "
                         "video fails the reference's patch-grid assert, :636)")


def features_per_sample(video_of, tokens):
    """The feature list `splice_into_text` indexes: it advances its feature index over text-only samples too (llava_arch.py:
    766-772, where the reference keeps a dummy feature per such sample), so the list has one entry per SAMPLE - the sample's
    video block, or None where nothing is read."""
    return [tokens[v] if v >= 0 else None for v in video_of]


def _narrow_heads(rm) -> bool:
    """heads of at most 128 columns - the widths the variable-length attention serves under autograd - or heads of 448 with
    `ops.set_attention_hd_varlen_train(True)` (a model without layers: nothing to ask)"""
    layers = getattr(rm, "layers", None)
    if not layers:
        return True
    hd = layers[0].memory_segment_fusion_attention.attention_head_size
    return hd <= 128 or (hd == 448 and ops.attention_hd_varlen_train())


def run_video_groups(model, videos, mem_prompt, frame_prompt, image_newline, with_frames=True, layout="one_token",
                     sizes=ROW_BATCH_SIZES, train=False, out=None, dst_rows=None, single=None, ragged=False, ragged_train=False,
                     clips=False, clips_train=False):
    """The memory path for several videos on the current stream - the ONE place that groups videos into row batches.
    `videos`: (pooled frame tokens [T, P, D], original frame indices [T] on the host) per video.  Videos with the same sampled
    frame count, dtype and device form a group (they share chunk bounds and fine-frame indices); `plan_row_batches` cuts it into
    row batches, each stepped by `recurrent_memory_transformer.row_batcher(size)` with per-video frame indices; the rest run as
    single videos on the model's own engine (`single(frames, idx, out)` -> tokens, default `video_memory_tokens`).
      out is None   -> returns the token blocks [rows_v, D] in input order (`train`: under autograd, through
                       video_memory_tokens_batched_train / the autograd path of video_memory_tokens)
      out, dst_rows -> inference: video v's block is written at row dst_rows[v] of the contiguous [out_rows, D] buffer `out`:
                       one emit per row batch (mavlm_fuse_emit_layout_batch_to), the `out=` slice for a single; returns None.
    `ragged` (LlavaMetaForCausalLM.enable_ragged_row_batches; inference - under autograd the grouping above stays): videos whose
    sampled length is a multiple of the 32-frame chunk are grouped by `plan_ragged_batches` instead - different chunk counts
    in one row batch, one ragged emit per group (`video_memory_tokens_batched(ragged=True)`); the rest as above.
    `ragged_train` (enable_ragged_row_batches(on, training=True)): with `train` the grouping comes from `plan_ragged_batches`
    too (same policy, same sizes) and a group runs through `video_memory_tokens_ragged_train`; without `train` it
    changes nothing.
    `clips` (LlavaMetaForCausalLM.enable_clip_row_batches; inference - under autograd it changes nothing): the videos of fewer
    than 32 sampled frames are grouped by `plan_clip_batches` first - different frame counts in ONE step, one emit per group
    (`video_memory_tokens_clips`); every other video goes through the grouping above.
    `clips_train` (enable_clip_row_batches(on, training=True)): with `train` the clips are grouped by `plan_clip_batches` too
    and a group runs through `video_memory_tokens_clips_train`; without `train` it changes nothing.  Heads of 448 columns:
    at that width it changes nothing either - the grouping stays the equal-length one - unless the process-wide switch
    `ops.set_attention_hd_varlen_train(True)` (off by default) is set: then the clips are grouped by `plan_clip_batches` too."""
    rm = model.recurrent_memory_transformer
    if (clips and not train) or (clips_train and train and _narrow_heads(rm)):
        cgroups, rest = plan_clip_batches([v[0].shape[0] for v in videos], [(v[0].dtype, str(v[0].device)) for v in videos], sizes)
        if cgroups:
            tokens = [None] * len(videos)
            for size, grp in cgroups:
                if train:
                    toks = video_memory_tokens_clips_train(model, rm.row_batcher(size), [videos[i][0] for i in grp],
                                                           [videos[i][1] for i in grp], mem_prompt, frame_prompt, image_newline,
                                                           with_frames, layout=layout)[0]
                    for j, i in enumerate(grp):
                        tokens[i] = toks[j]
                    continue
                toks = video_memory_tokens_clips(model, rm.row_batcher(size), [videos[i][0] for i in grp], [videos[i][1] for i in grp],
                                                 mem_prompt, frame_prompt, image_newline, with_frames, out=out, layout=layout,
                                                 dst_rows=None if out is None else [dst_rows[i] for i in grp])[0]
                if out is None:
                    for j, i in enumerate(grp):
                        tokens[i] = toks[j]
            sub = run_video_groups(model, [videos[i] for i in rest], mem_prompt, frame_prompt, image_newline, with_frames, layout,
                                   sizes, train, out, None if out is None else [dst_rows[i] for i in rest], single, ragged,
                                   ragged_train) if rest else []
            if out is not None:
                return None
            for j, i in enumerate(rest):
                tokens[i] = sub[j]
            return tokens
    groups = []
    if (ragged and not train) or (ragged_train and train):
        groups, batches, singles = plan_ragged_batches([v[0].shape[0] for v in videos], 32,
                                                       [(v[0].dtype, str(v[0].device)) for v in videos], sizes)
    else:
        batches, singles = plan_row_batches([(v[0].shape[0], v[0].dtype, str(v[0].device)) for v in videos], sizes)
    if single is None:
        def single(frames, idx, o):
            return video_memory_tokens(model, frames, idx, mem_prompt, frame_prompt, image_newline, with_frames, out=o,
                                       layout=layout)[0]
    tokens = [None] * len(videos)
    for size, grp in groups:
        bp = rm.row_batcher(size)
        if train:
            toks = video_memory_tokens_ragged_train(model, bp, [videos[i][0] for i in grp], [videos[i][1] for i in grp],
                                                    mem_prompt, frame_prompt, image_newline, with_frames, layout=layout)[0]
            for j, i in enumerate(grp):
                tokens[i] = toks[j]
            continue
        toks = video_memory_tokens_batched(model, bp, [videos[i][0] for i in grp], [videos[i][1] for i in grp], mem_prompt,
                                           frame_prompt, image_newline, with_frames, out=out, layout=layout,
                                           dst_rows=None if out is None else [dst_rows[i] for i in grp], ragged=True)[0]
        if out is None:
            for j, i in enumerate(grp):
                tokens[i] = toks[j]
    for grp in batches:
        bp = rm.row_batcher(len(grp))
        frames, idxs = [videos[i][0] for i in grp], [videos[i][1] for i in grp]
        if train:
            toks = video_memory_tokens_batched_train(model, bp, frames, idxs, mem_prompt, frame_prompt, image_newline,
                                                     with_frames, layout=layout)[0]
        elif out is not None:
            video_memory_tokens_batched(model, bp, frames, idxs, mem_prompt, frame_prompt, image_newline, with_frames, out=out,
                                        layout=layout, dst_rows=[dst_rows[i] for i in grp])
            continue
        else:
            toks = video_memory_tokens_batched(model, bp, frames, idxs, mem_prompt, frame_prompt, image_newline, with_frames,
                                               layout=layout)[0]
        for j, i in enumerate(grp):
            tokens[i] = toks[j]
    for i in singles:
        frames, idx = videos[i]
        if out is not None:
            rows = video_token_rows(frames.shape[0], rm.num_memory_tokens, rm.patch_size, with_frames,
                                    cache_cap=getattr(rm.config, "cache_cap", 10), n_mem_prompt=mem_prompt.shape[0],
                                    n_frame_prompt=frame_prompt.shape[0], layout=layout)
            single(frames, idx, out[dst_rows[i]:dst_rows[i] + rows])
        else:
            tokens[i] = single(frames, idx, None)
    return None if out is not None else tokens


def _tail_wants_grad(model, *tensors) -> bool:
    """Can anything AFTER the recurrent steps receive a gradient?  (`memory_fuser`, `token_type_embedding`, and the
    tensors the caller hands in: prompt embeddings of a trainable `embed_tokens`, `image_newline`.)"""
    if not torch.is_grad_enabled():
        return False
    mods = (getattr(model, "memory_fuser", None), getattr(model, "token_type_embedding", None))
    return any(p.requires_grad for m in mods if m is not None for p in m.parameters()) or \
        any(t is not None and t.requires_grad for t in tensors)


def path_wants_grad(model, *tensors) -> bool:
    """Any gradient consumer on the memory path: the recurrent transformer or the tail (see _tail_wants_grad)."""
    return torch.is_grad_enabled() and (any(p.requires_grad for p in model.recurrent_memory_transformer.parameters())
                                        or _tail_wants_grad(model, *tensors))


def _lay_out_block(block, nl, layout, patches):
    """A [rows, D] block in a token layout, as torch ops: the feature rows are copied (the same bits in every layout), the
    newline rows are an expand of `nl` [1, D], whose backward sums the gradient of every inserted row (llava_arch.py:338,355)."""
    g = layout_period(layout, patches)
    if g:
        b = block.reshape(-1, g, block.shape[-1])
        return torch.cat((b, nl.expand(b.shape[0], 1, b.shape[-1])), dim=1).reshape(-1, block.shape[-1])
    return torch.cat((block, nl), dim=0) if layout == "one_token" else block


def _train_tail_operands(image_newline, memory_prompt_embeds, frame_prompt_embeds, layout, x):
    """(newline row [1, D] or None, memory prompt, frame prompt) in the dtype of the PE frames `x`, for `_train_block`"""
    _require_newline(image_newline, layout)
    nl = None if layout == "no_token" else image_newline.to(device=x.device, dtype=x.dtype).reshape(1, x.shape[2])
    return nl, memory_prompt_embeds.to(x.dtype), frame_prompt_embeds.to(x.dtype)


def _train_block(model, fused, x, fine_cpu, mp, fp, nl, with_frames, layout):
    """One video's token block under autograd (llava_arch.py:513-524,554,567-634) from its fused memory rows [n * R, D], oldest
    first, and its PE frames `x`: the type-embedding add of the fine frames, the layout and the concatenation are torch ops, so
    autograd routes the gradients of token_type_embedding, the prompt embeddings and image_newline exactly as in the reference."""
    P, D = x.shape[1:]
    parts = [mp, _lay_out_block(fused, nl, layout, P)]                                     # :567-634
    if with_frames:
        temb = model.token_type_embedding.weight
        fine = x[_device_indices(fine_cpu, x.device)] + temb[1].to(x.dtype)                # :513-524,554
        parts += [fp, _lay_out_block(fine.reshape(-1, D), nl, layout, P)]
    return torch.cat(parts, dim=0)


def _video_memory_tokens_autograd(model, rm, x, fine_cpu, memory_prompt_embeds, frame_prompt_embeds, image_newline,
                                  with_frames, out, layout="one_token"):
    """Training-mode tail of video_memory_tokens (llava_arch.py:545-554,567-634): the fuser MLP runs as HIP autograd
    Functions - without `fused_gelu`, which the row-batched tails pass -, then `_train_block`."""
    from .. import _autograd as ag
    P, D = x.shape[1], x.shape[2]
    # engine-mode cache entries are ring views: torch.cat copies them (the graph must not alias the ring)
    mem = torch.cat(rm.memory_cache, dim=0)                                               # :545
    fused = ag.fuser_mlp(model.memory_fuser, mem, model.token_type_embedding.weight[0]).reshape(-1, D)        # :546-553
    nl, mp, fp = _train_tail_operands(image_newline, memory_prompt_embeds, frame_prompt_embeds, layout, x)
    tokens = _train_block(model, fused, x, fine_cpu, mp, fp, nl, with_frames, layout)
    if out is not None:
        raise capi.MavlmError("video_memory_tokens: `out=` is an inference-path feature (no autograd through a "
                              "caller-owned buffer)")
    info = {"num_memories": len(rm.memory_cache), "pe_frames": x, "fine_idx": fine_cpu,
            "memory_rows": _memory_rows(memory_prompt_embeds.shape[0], len(rm.memory_cache), rm.num_memory_tokens * P, layout, P)}
    return tokens, info


_SIDE_STREAMS = {}


def _side_streams(device_index: int, n: int):
    """The first n side streams of a device, shared by every pool of the process.  HIP multiplexes its streams onto a few
    hardware queues (4 by default): a second pool with streams of its own ended up sharing queues and ran its two videos
    one after the other (measured at M = 8: 2.11 instead of 1.50 ms per pair of videos after another pool had been used)."""
    have = _SIDE_STREAMS.setdefault(device_index, [])
    while len(have) < n:
        have.append(torch.cuda.Stream(device=device_index))
    return have[:n]


class MemoryPathPool:
    """Keeps `n` videos in flight on `n` HIP streams over ONE set of weights.

    Why: at the reference shapes every kernel of the path launches a grid that is not a multiple of the 256 CUs
    (M*196 rows -> 1.5 / 3.06 "rounds"), so ~23 % of each kernel runs on a partly idle chip.  Kernels of an
    independent video on another stream fill those tails (measured +21 % frames/s with 2 videos in flight).
    Videos are independent units (the recurrence is per video), so results are bit-identical to the serial path.

    usage:  pool = MemoryPathPool(model, 2)
            outs = pool.run([(frames0, idx0), (frames1, idx1), ...], mem_prompt, frame_prompt, newline)
    (`layout=`: the token layout of every block, as video_memory_tokens)

    `batch` > 1 (round 3): each stream steps `batch` videos TOGETHER as a row batch (`BatchedProjector`: the memory rows of
    the videos stacked into every weight-shared GEMM / LayerNorm launch) instead of one.  Consecutive videos of equal length
    and equal frame indices form a batch; whatever does not fill one runs through the single-video slots.  At the
    reference's 8 memory tokens this is what fills the chip (1568-row operands otherwise).
    """

    def __init__(self, model, n: int = 2, batch: int = 1):
        rm = model.recurrent_memory_transformer
        self.model = model
        # More than LN_MAX_STREAMS streams: the forward-progress argument of the fused dense + residual + LayerNorm kernel
        # (waiting workgroups per XCD, include/mavlm.h MAVLM_LN_MAX_STREAMS) no longer covers the pool - every slot of such
        # a pool runs the two-kernel form (GEMM + row LayerNorm; same fp32 inputs, statistics added in another order), on
        # recurrent states of its own (the model's own engine keeps the fused form for serial use).
        self.fused_ln_never = n > capi.LN_MAX_STREAMS
        if self.fused_ln_never:
            self.slots = [_ReplicaView(model, rm.spawn_replica(fused_ln_never=True)) for _ in range(n)]
        else:
            self.slots = [model] + [_ReplicaView(model, rm.spawn_replica()) for _ in range(n - 1)]
        self.batch = int(batch)
        self.bslots = [BatchedProjector(rm, self.batch, fused_ln_never=self.fused_ln_never) for _ in range(n)] if self.batch > 1 else []
        self.streams = None

    @torch.no_grad()           # inference feature: the replicas' FIFOs are ring views, not autograd tensors
    def run(self, videos, memory_prompt_embeds, frame_prompt_embeds, image_newline, with_frames: bool = True,
            layout: str = "one_token"):
        if self.streams is None:
            self.streams = _side_streams(torch.cuda.current_device(), len(self.slots))
        cur = torch.cuda.current_stream()
        for st in self.streams:
            st.wait_stream(cur)
        outs = [None] * len(videos)
        singles = list(range(len(videos)))
        if self.batch > 1:
            # groups of `batch` consecutive videos with the same shape and frame indices step together
            singles, i, g = [], 0, 0
            while i < len(videos):
                grp = videos[i:i + self.batch]
                same = len(grp) == self.batch and all(v[0].shape == grp[0][0].shape and torch.equal(v[1], grp[0][1])
                                                      for v in grp[1:])
                if not same:
                    singles.append(i)
                    i += 1
                    continue
                k = g % len(self.bslots)
                with torch.cuda.stream(self.streams[k]):
                    toks = video_memory_tokens_batched(self.model, self.bslots[k], [v[0] for v in grp], grp[0][1],
                                                       memory_prompt_embeds, frame_prompt_embeds, image_newline, with_frames,
                                                       layout=layout)[0]
                    for j, v in enumerate(grp):
                        outs[i + j] = toks[j]
                        v[0].record_stream(self.streams[k])
                i += self.batch
                g += 1
        for j, i in enumerate(singles):
            frames, idx_cpu = videos[i]
            k = j % len(self.slots)
            with torch.cuda.stream(self.streams[k]):
                outs[i] = video_memory_tokens(self.slots[k], frames, idx_cpu, memory_prompt_embeds, frame_prompt_embeds,
                                              image_newline, with_frames, layout=layout)[0]
                frames.record_stream(self.streams[k])
        for st in self.streams:
            cur.wait_stream(st)
        return outs


class GraphedVideoMemory:
    """hipGraph-captured memory path for one video shape (T frames): PE add, every chunk step (evolution +
    formation, FIFO slots baked in), fuser MLP + type add + concat - ONE graph launch per video instead of ~45 kernel
    launches (BASELINE.json configs[2]: "hipGraph-captured per-chunk memory update").  Possible because no entry
    point of the C ABI allocates or synchronises and the recurrent state lives in caller-owned buffers.

    usage:  g = GraphedVideoMemory(model, T=256, frame_idx_cpu=idx)        # captures on the current device
            tokens = g(frames, mem_prompt, frame_prompt, newline)          # copies into the static inputs, replays
    The returned tensor is the graph's static output buffer (valid until the next call).  A new shape (T, indices,
    with_frames, layout) needs a new instance: the token layout is baked into the captured launches.

    A graph replays the device pointers it was captured with: the engine's workspace and FIFO ring, its packed weight copies
    (fp32 biases / LayerNorm affines, concatenated K/V weights), the PE table, the fuser and token-type parameters.  The instance
    holds the engine and its packed copies, so those stay allocated while it lives, and before every replay it runs on the host
    (no device sync) the staleness check an eager video start runs: a weight update (in place, `load_state_dict`, through `.data`
    after a `train()` phase), `bind_fuser`, `.to()` / `.half()` of the module, or an engine re-created for a longer chunk makes
    `__call__` raise MavlmError naming what changed instead of replaying.  Build a new instance then (`enable_memory_graphs` does
    so by itself)."""

    @torch.no_grad()
    def __init__(self, model, T: int, frame_idx_cpu: torch.Tensor, with_frames: bool = True, slot=None,
                 layout: str = "one_token"):
        rm = model.recurrent_memory_transformer
        self.layout = layout
        self.view = slot if slot is not None else _ReplicaView(model, rm.spawn_replica())
        self.idx = frame_idx_cpu.clone()
        self.with_frames = with_frames
        p = next(rm.parameters())
        D, P = rm.hidden_size, rm.patch_size
        dev, dt = p.device, p.dtype
        self.x = torch.zeros((T, P, D), device=dev, dtype=dt)
        self.mp = torch.zeros((len(MEMORY_PROMPT_IDS), D), device=dev, dtype=dt)
        self.fp = torch.zeros((len(FRAME_PROMPT_IDS), D), device=dev, dtype=dt)
        self.nl = torch.zeros((D,), device=dev, dtype=dt)
        # warm-up outside capture: engine creation, weight packing, kernel attribute calls, index uploads.  Its eager steps also
        # wait for (and clear) a K/V projection left pending by a discarded `project_ahead`, which a captured step would refuse.
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            video_memory_tokens(self.view, self.x, self.idx, self.mp, self.fp, self.nl, with_frames, layout=layout)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out, _ = video_memory_tokens(self.view, self.x, self.idx, self.mp, self.fp, self.nl, with_frames, layout=layout)
        # what the module's host-side state looks like after this video (ring views of the FIFO, scores of the chunks): a replay
        # only re-runs the device work, so __call__ puts these back - `recurrent_memory_transformer.memory_cache` read after a
        # replayed forward is the replayed video's cache, as after an eager forward (matters when the slot is the model itself)
        rm_ = self.view.recurrent_memory_transformer
        self._cache = list(rm_.memory_cache)
        # what the graph reads: held (the captured pointers stay allocated) and compared before every replay (stale())
        self._dev, self._dt = dev, dt
        self._engine = rm_._engine
        self._keep = self._engine.keep
        self._version = self._engine.version
        self._epoch = rm_._packed_epoch
        self._ptrs = self._outside_ptrs()
        # (and the device index vectors it reads: _INDEX_CACHE may drop its references to them)
        self._idx_dev = (_device_indices(self.idx, dev), _device_indices(fine_frame_indices(T), dev))

    def _outside_ptrs(self):
        """pointers of the tensors the graph reads beside the engine: the PE table, the fuser and token-type parameters"""
        v = self.view
        return (v.positional_encoding.table().data_ptr(),) + tuple(
            p.data_ptr() for m in (v.memory_fuser, v.token_type_embedding) for p in m.parameters())

    def stale(self) -> Optional[str]:
        """None if a replay computes what an eager video would, else what changed since the capture.  Host only: the
        staleness protocol of an eager video start (`memory_cache = []`, then `engine()`: re-packs what changed), then a
        comparison with what the graph was captured with."""
        rm = self.view.recurrent_memory_transformer
        p = next(rm.parameters())
        if p.dtype != self._dt or p.device != self._dev:
            return "the module was cast to another dtype or moved"
        if rm._engine is not None and rm._weights_maybe_stale():
            rm._engine.version = None
        eng = rm.engine(self._dev, self._dt)
        if eng is not self._engine:
            return "the engine was re-created (module moved / cast, or a longer chunk)"
        if eng.keep is not self._keep or eng.version != self._version or rm._packed_epoch != self._epoch:
            return "the weights were re-packed (parameter update, load_state_dict, train() phase or bind_fuser)"
        if self._outside_ptrs() != self._ptrs:
            return "the PE table, memory_fuser or token_type_embedding tensors were replaced"
        return None

    @torch.no_grad()
    def __call__(self, frames, memory_prompt_embeds, frame_prompt_embeds, image_newline):
        why = self.stale()
        if why is not None:
            raise capi.MavlmError(f"GraphedVideoMemory: stale graph, not replayed: {why} since the capture - build a new one")
        return self._replay(frames, memory_prompt_embeds, frame_prompt_embeds, image_newline)

    def _replay(self, frames, memory_prompt_embeds, frame_prompt_embeds, image_newline):
        self.x.copy_(frames)
        self.mp.copy_(memory_prompt_embeds)
        self.fp.copy_(frame_prompt_embeds)
        if self.layout != "no_token":
            _require_newline(image_newline, self.layout)
            self.nl.copy_(image_newline)
        self.graph.replay()
        self.view.recurrent_memory_transformer._memory_cache = list(self._cache)
        return self.out


class _ReplicaView:
    """The four memory sub-modules as seen by one pool slot (shared weights, private recurrent state)."""

    def __init__(self, model, projector):
        self.positional_encoding = model.positional_encoding
        self.memory_fuser = model.memory_fuser
        self.token_type_embedding = model.token_type_embedding
        self.recurrent_memory_transformer = projector


class LlavaMetaForCausalLM:
    """Mixin for the *ForCausalLM wrapper: needs `get_model()`, `.config`, `.device`."""

    def get_model(self):
        raise NotImplementedError

    def get_vision_tower(self):
        return self.get_model().get_vision_tower()

    def get_2dPool(self, image_feature, stride=2):
        """[F, side*side, D] -> [F, ceil(side/stride)^2, D]  (llava_arch.py:277-297).  Step before the path
        (SURVEY.md §8f rank 1).  The bilinear mode the reference scripts use runs as a HIP kernel on 16-bit GPU
        tensors (no NCHW permute round trip); the average / max modes stay backbone ops."""
        side = self.get_vision_tower().num_patches_per_side
        nf, _, nd = image_feature.shape
        mode = self.config.mm_spatial_pool_mode
        if mode == "bilinear" and image_feature.is_cuda and image_feature.dtype in (torch.bfloat16, torch.float16) \
                and nd % 8 == 0:
            return ops.pool_bilinear(image_feature.contiguous(), side, stride)      # HIP kernel (channels stay last)
        x = image_feature.view(nf, side, side, -1).permute(0, 3, 1, 2).contiguous()
        if mode == "average":
            x = nn.functional.avg_pool2d(x, stride)
        elif mode == "max":
            x = nn.functional.max_pool2d(x, stride)
        elif mode == "bilinear":
            size = [math.ceil(side / stride), math.ceil(side / stride)]
            x = nn.functional.interpolate(x, size=size, mode="bilinear")
        else:
            raise ValueError(f"Unexpected mm_spatial_pool_mode: {mode}")
        return x.permute(0, 2, 3, 1).reshape(nf, -1, nd)

    def encode_images(self, images):
        feats = self.get_model().get_vision_tower()(images)
        return self.get_model().mm_projector(feats).detach()      # llava_arch.py:299-304

    def get_synced_dropout_decision(self, prob: float = 0.5):
        """Shared Bernoulli(prob) across ranks (llava_arch.py:378-386): rank-0 draw, 1-element broadcast."""
        if not dist.is_initialized():
            return torch.rand(1).item() < prob
        flag = torch.zeros(1, device=self.device)
        if dist.get_rank() == 0:
            flag.fill_(1.0 if torch.rand(1).item() < prob else 0.0)
        dist.broadcast(flag, src=0)
        return bool(flag.item())

    def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels,
                                             images, modalities=["image"], image_sizes=None):
        vision_tower = self.get_vision_tower()
        if vision_tower is None or images is None or input_ids.shape[1] == 1:
            return input_ids, position_ids, attention_mask, past_key_values, None, labels        # :392-394
        if isinstance(modalities, str):
            modalities = [modalities]
        model = self.get_model()
        if not (type(images) is list or images.ndim == 5):
            # A plain [N,3,H,W] image batch (llava_arch.py:703): the reference encodes it and then - its prompt insertion is
            # unconditional (:705-731) - uses the features of image 0 as "memory" and of image 1 as "frames" (an IndexError
            # for a single image).  Backbone ops only; restated as it behaves.
            feats = self.encode_images(images)                                                       # :703
            dev = feats.device
            mem_prompt = model.embed_tokens(torch.tensor([MEMORY_PROMPT_IDS], device=dev)).squeeze(0)
            frame_prompt = model.embed_tokens(torch.tensor([FRAME_PROMPT_IDS], device=dev)).squeeze(0)
            drop = self.get_synced_dropout_decision(prob=0.5) and bool(getattr(self, "training", False)) and \
                bool(getattr(self.config, "dropout_frames", False))                                  # :719-720
            if drop:
                tokens = torch.cat((mem_prompt, feats[0]), dim=0)                                    # :722-725
            else:
                tokens = torch.cat((mem_prompt, feats[0], frame_prompt, feats[1]), dim=0)            # :729-731
            return splice_into_text(self, model, [tokens], input_ids, position_ids, attention_mask, past_key_values, labels)
        images = [x.unsqueeze(0) if x.ndim == 3 else x for x in images] if type(images) is list else list(images)
        vids = [i for i in range(min(len(modalities), len(images))) if modalities[i] == "video"]     # :403-406
        if not vids:
            # the reference: every non-video entry is skipped by the memory loop (:487-490), `image_features` ends up empty
            # and the prompt insertion indexes it (:722 / :730)
            raise IndexError("list index out of range (no video among `images`: the reference's memory branch skips "
                             "non-video entries, llava_arch.py:487-490, and then indexes an empty feature list, :730)")
        if len(vids) != 1:
            return self._prepare_videos(model, [images[i] for i in vids], input_ids, position_ids, attention_mask,
                                        past_key_values, labels)
        # non-video entries beside the video are encoded and then DROPPED by the reference (:487-490, 556): dropped here too
        images = [images[vids[0]]]
        layout = token_layout(self.config)                                                      # :562-634
        _require_newline(getattr(model, "image_newline", None), layout)                         # AttributeError, as the reference
        video = images[0]
        idx_cpu = sample_frame_indices(video.shape[0])                                          # :437-451
        feats = self.encode_images(video[idx_cpu.to(video.device)])                             # :457-481
        pooled = self.get_2dPool(feats)                                                         # :495
        dev = pooled.device
        mem_prompt = model.embed_tokens(torch.tensor([MEMORY_PROMPT_IDS], device=dev)).squeeze(0)   # :708-709
        frame_prompt = model.embed_tokens(torch.tensor([FRAME_PROMPT_IDS], device=dev)).squeeze(0)  # :714-715
        training = bool(getattr(self, "training", False))
        dropout_frames = getattr(self.config, "dropout_frames", False)
        # :719 - called on EVERY forward, inference included, exactly as the reference: without a process group one local
        # draw; with one, rank 0 draws and every rank joins the 1-element broadcast (ranks of the reference and of this
        # build can therefore be mixed in one job, and the RNG streams of the non-zero ranks stay the reference's)
        drop = self.get_synced_dropout_decision(prob=0.5) and training and bool(dropout_frames)   # :720
        # Step after the path.  Fast path = what the reference's memory branch supports anyway
        # (batch 1, one image placeholder, llava_arch.py:436): the final [1, L, D] buffer is allocated once and the
        # HIP path writes the video block straight into it; everything else goes through the general splice.
        direct = self._direct_emit(model, pooled, idx_cpu, mem_prompt, frame_prompt, not drop, input_ids, position_ids,
                                   attention_mask, past_key_values, labels, layout)
        if direct is not None:
            return direct
        tokens = self._video_tokens(model, pooled, idx_cpu, mem_prompt, frame_prompt, not drop, layout=layout)
        return splice_into_text(self, model, [tokens], input_ids, position_ids, attention_mask, past_key_values, labels)

    # -- several videos per forward: one per sample, equal lengths stepped together as row batches ------------------------
    row_batch_sizes = ROW_BATCH_SIZES        # sizes a group of equal-length videos is cut into (plan_row_batches); overridable

    def _prepare_videos(self, model, videos, input_ids, position_ids, attention_mask, past_key_values, labels):
        """`prepare_inputs_labels_for_multimodal` for V >= 2 videos: exactly V samples hold an image token, one each, and the
        k-th of them takes the k-th video; the other samples are text only.  The result is what padding the single-sample
        calls together gives (`splice_into_text`).  Videos of equal sampled length step together (`run_video_groups`); without a
        gradient consumer every block is emitted straight into the padded buffer; the hipGraph cache steps aside."""
        mask = torch.ones_like(input_ids, dtype=torch.bool) if attention_mask is None else attention_mask.bool()
        ids_list = [i[m] for i, m in zip(input_ids, mask)]
        ids_host = [i.tolist() for i in ids_list]
        per_sample = [sum(t == IMAGE_TOKEN_INDEX for t in ids) for ids in ids_host]
        if any(c > 1 for c in per_sample) or sum(per_sample) != len(videos):
            raise NotImplementedError(_ONE_VIDEO_PER_SAMPLE)                 # (before anything is encoded)
        layout = token_layout(self.config)                                                      # :562-634
        newline = getattr(model, "image_newline", None)
        _require_newline(newline, layout)
        vids = []
        for video in videos:                                   # per video, as the single-video branch does
            idx_cpu = sample_frame_indices(video.shape[0])                                      # :437-451
            pooled = self.get_2dPool(self.encode_images(video[idx_cpu.to(video.device)]))       # :457-481,495
            vids.append((pooled, idx_cpu))
        dev, dt, D = vids[0][0].device, vids[0][0].dtype, vids[0][0].shape[-1]
        mem_prompt = model.embed_tokens(torch.tensor([MEMORY_PROMPT_IDS], device=dev)).squeeze(0)   # :708-709
        frame_prompt = model.embed_tokens(torch.tensor([FRAME_PROMPT_IDS], device=dev)).squeeze(0)  # :714-715
        # :719-720 - ONE draw per forward (one broadcast with a process group), applied to every video of the forward
        drop = self.get_synced_dropout_decision(prob=0.5) and bool(getattr(self, "training", False)) and \
            bool(getattr(self.config, "dropout_frames", False))
        rm = model.recurrent_memory_transformer
        rows = [video_token_rows(p.shape[0], rm.num_memory_tokens, rm.patch_size, not drop,
                                 cache_cap=getattr(rm.config, "cache_cap", 10), layout=layout) for p, _ in vids]
        plan = VideoPlacement(ids_host, rows, getattr(self.config, "tokenizer_padding_side", "right") == "left",
                              getattr(self.config, "tokenizer_model_max_length", None))
        train = path_wants_grad(model, mem_prompt, frame_prompt, newline)
        if train or plan.general or not vids[0][0].is_cuda or any(p.device != dev or p.dtype != dt for p, _ in vids):
            tokens = run_video_groups(model, vids, mem_prompt, frame_prompt, newline, not drop, layout, self.row_batch_sizes,
                                      train=train, ragged=self._ragged_row_batches and not train,
                                      ragged_train=self._ragged_row_batches_train and train,
                                      clips=self._clip_row_batches and not train,
                                      clips_train=self._clip_row_batches_train and train)
            return splice_into_text(self, model, features_per_sample(plan.video_of, tokens), input_ids, position_ids,
                                    attention_mask, past_key_values, labels)
        # in place: the padded buffer once, text rows from embed_tokens, padding zeroed, every block emitted where it belongs
        B, L = len(ids_list), plan.Lmax
        emb = torch.empty((B, L, D), device=dev, dtype=dt)
        for s, lo, hi in plan.padding:
            emb[s, lo:hi].zero_()
        text = model.embed_tokens(torch.cat([ids_list[s][lo:hi] for s, lo, hi, _ in plan.segments])) if plan.segments else None
        at = 0
        for s, lo, hi, row in plan.segments:
            emb[s, row:row + hi - lo] = text[at:at + hi - lo].to(dt)
            at += hi - lo
        with torch.no_grad():
            run_video_groups(model, vids, mem_prompt, frame_prompt, newline, not drop, layout, self.row_batch_sizes,
                             out=emb.view(B * L, D), dst_rows=plan.dst_row, ragged=self._ragged_row_batches,
                             clips=self._clip_row_batches)
        if text is not None and text.dtype != dt:
            emb = emb.to(text.dtype)
        lab_list = None if labels is None else [l[m] for l, m in zip(labels, mask)]
        out_labels, out_mask, out_pos = plan.labels_mask_positions(lab_list, attention_mask, position_ids)
        return None, _pos_skipping(self, out_pos, emb), out_mask, past_key_values, emb, out_labels

    _ragged_row_batches = False
    _ragged_row_batches_train = False

    def enable_ragged_row_batches(self, on: bool = True, training: bool = False):
        """Several videos per forward: let a row batch hold videos of DIFFERENT lengths (off by default).  Off, videos step
        together only when their sampled frame counts are equal (`plan_row_batches`); everything else runs as single videos.
        On, every video whose sampled length is a multiple of the 32-frame chunk - the sampler turns every video of 32 or more
        frames into one - is grouped by `plan_ragged_batches`: up to 8 videos whose chunk counts differ by at most a factor of
        two share one row-batched engine, ordered longest first and stepped as a shrinking prefix, with one ragged emit per
        group into the padded `inputs_embeds`.  Inference; a forward that records a graph keeps the grouping of the switch off.
        The hipGraph cache and `MemoryPathPool` are not affected.
        `training=True` additionally groups the videos of a forward under autograd that way (off by default, also with `on`):
        a group steps through `BatchedProjector.step_train(ragged=True)`, forward and backward of its active videos in one pass
        per step; `on=False` switches both off."""
        self._ragged_row_batches = bool(on)
        self._ragged_row_batches_train = bool(on) and bool(training)

    _clip_row_batches = False
    _clip_row_batches_train = False

    def enable_clip_row_batches(self, on: bool = True, training: bool = False):
        """Several videos per forward: let the videos of FEWER than 32 frames share a row batch (off by default).  Such a video
        is one chunk of all its frames, so two of them step together only when their frame counts are equal; everything else
        runs as single videos.  On, they are grouped by `plan_clip_batches`: up to 8 clips whose lengths differ by at most a
        factor of two share one row-batched engine and take ONE step with a frame count per video (`mavlm_step_batch_frames`),
        then one emit per group into the padded `inputs_embeds`.  Inference; a forward that records a graph keeps the
        grouping of the switch off.  Independent of `enable_ragged_row_batches` (which serves the videos of 32 frames and more).
        The other row-batched emits take every hidden size that is a multiple of 128; the clip emit (a fine-frame count per
        video, `mavlm_fuse_emit_layout_frames_to`) still needs a multiple of 256 (D = 896: `MavlmError` before any step).
        Measured 1.23 x at D = 1024 and 0.96 x (slower) at D = 3584 with 4 clips: hence off by default.
        At heads of 448 columns (D = 3584) a clip step runs one attention launch per video; the process-wide switch
        `_ops.set_attention_hd_varlen(True)` (`mavlm_set_attention_hd_varlen`, OFF by default, same bits) makes it one
        variable-length launch per formation layer - measured 1.10 x against single videos with those 4 clips.  This method does
        not touch that switch.
        `training=True` additionally groups the clips of a forward under autograd that way (off by default, also with `on`): a
        group takes one `BatchedProjector.step_train_frames` - the variable-length attention forward and backward - and
        `video_memory_tokens_clips_train` builds its blocks, at every hidden size of the training path (896 included).  Heads
        of 448 columns: the training grouping stays as it is with the switch off unless `_ops.set_attention_hd_varlen_train(True)`
        (process-wide, OFF by default; this method does not touch it) - then the step runs the variable-length 448 forward and its
        backward `mavlm_attention_bwd_hd_batch_varlen`.  `on=False` switches both off."""
        self._clip_row_batches = bool(on)
        self._clip_row_batches_train = bool(on) and bool(training)

    # -- hipGraph replay for repeated video shapes (round 4) -------------------------------------------------------------
    def enable_memory_graphs(self, capacity: int = 4):
        """Inference: serve videos of a shape seen before ((frames, frame indices, with_frames, token layout) of the sampled video) by replaying
        a captured hipGraph of the whole per-video launch sequence (`GraphedVideoMemory` on the model's own engine: PE add,
        every chunk step, fuser + emit) instead of ~45 launches; the first occurrence of a shape runs eagerly, the second
        captures.  Bit-identical to the eager path (`test_graph_capture_replay_bit_identical`); a graph captured over weights or an
        engine that have changed since is dropped and captured again (`GraphedVideoMemory.stale`, tests/test_gpu_replay_coherence.py).
        Training-mode modules run eagerly.  `capacity` graphs are kept
        (least recently used out); 0 switches the cache off.  Each graph holds static copies of its input frames and of its
        token block."""
        self._mem_graph_capacity = int(capacity)
        self._mem_graphs = {}
        self._mem_graph_seen = {}

    def _video_tokens(self, model, pooled, idx_cpu, mem_prompt, frame_prompt, with_frames, out=None, layout="one_token"):
        """video_memory_tokens, through the graph cache when it applies (inference, shape seen before)"""
        cap = getattr(self, "_mem_graph_capacity", 0)
        newline = getattr(model, "image_newline", None)
        if (cap <= 0 or path_wants_grad(model, mem_prompt, frame_prompt, newline)
                or torch.cuda.is_current_stream_capturing() or model.recurrent_memory_transformer.training
                or getattr(model.recurrent_memory_transformer, "record_attention_maps", False)):      # (maps: eager steps only)
            return video_memory_tokens(model, pooled, idx_cpu, mem_prompt, frame_prompt, newline, with_frames, out=out,
                                       layout=layout)[0]
        key = (pooled.shape[0], tuple(int(i) for i in idx_cpu.tolist()), bool(with_frames), pooled.dtype, pooled.device.index)
        if layout != "one_token":
            key += (layout,)                               # (a graph is captured for ONE layout; the default keeps the plain key)
        g = self._mem_graphs.pop(key, None)
        if g is not None and g.stale() is not None:
            g = None                                       # captured over state that has changed since: dropped, re-captured
        if g is None:
            n = self._mem_graph_seen.get(key, 0) + 1
            self._mem_graph_seen[key] = n
            if len(self._mem_graph_seen) > 64:
                self._mem_graph_seen.pop(next(iter(self._mem_graph_seen)))
            if n < 2:
                return video_memory_tokens(model, pooled, idx_cpu, mem_prompt, frame_prompt, newline, with_frames,
                                           out=out, layout=layout)[0]
            with torch.no_grad():
                g = GraphedVideoMemory(model, pooled.shape[0], idx_cpu, with_frames, slot=model, layout=layout)
            while len(self._mem_graphs) >= cap:
                self._mem_graphs.pop(next(iter(self._mem_graphs)))
        self._mem_graphs[key] = g                          # (re-inserted last: most recently used)
        with torch.no_grad():
            tokens = g._replay(pooled, mem_prompt, frame_prompt, newline)                 # (validated above / just captured)
        if out is not None:
            out.copy_(tokens)
            return out
        return tokens.clone()                              # (the graph's static buffer is overwritten by its next replay)

    def _direct_emit(self, model, pooled, idx_cpu, mem_prompt, frame_prompt, with_frames, input_ids, position_ids,
                     attention_mask, past_key_values, labels, layout="one_token"):
        if input_ids.shape[0] != 1:
            return None
        if path_wants_grad(model, mem_prompt, frame_prompt, getattr(model, "image_newline", None)):
            return None                                    # training: tokens must stay in the autograd graph
        mask = torch.ones_like(input_ids, dtype=torch.bool) if attention_mask is None else attention_mask.bool()
        ids = input_ids[0][mask[0]]
        pos = torch.where(ids == IMAGE_TOKEN_INDEX)[0].tolist()
        if len(pos) != 1:
            return None
        p = pos[0]
        rm = model.recurrent_memory_transformer
        rows = video_token_rows(pooled.shape[0], rm.num_memory_tokens, rm.patch_size, with_frames,
                                cache_cap=getattr(rm.config, "cache_cap", 10), layout=layout)
        n_text = ids.shape[0] - 1
        total = n_text + rows
        max_tok = getattr(self.config, "tokenizer_model_max_length", None)
        if max_tok is not None and total > max_tok:
            return None                                    # truncation cuts into the block: general path
        text = model.embed_tokens(torch.cat([ids[:p], ids[p + 1:]]))
        emb = torch.empty((1, total, pooled.shape[-1]), device=pooled.device, dtype=pooled.dtype)
        emb[0, :p] = text[:p].to(emb.dtype)
        emb[0, p + rows:] = text[p:].to(emb.dtype)
        self._video_tokens(model, pooled, idx_cpu, mem_prompt, frame_prompt, with_frames, out=emb[0, p:p + rows], layout=layout)
        if text.dtype != emb.dtype:
            emb = emb.to(text.dtype)
        out_labels = None
        if labels is not None:
            lab = labels[0][mask[0]]
            out_labels = torch.cat([lab[:p], torch.full((rows,), IGNORE_INDEX, device=lab.device, dtype=lab.dtype),
                                    lab[p + 1:]])[None]
        out_mask = None if attention_mask is None else torch.ones((1, total), device=attention_mask.device,
                                                                  dtype=attention_mask.dtype)
        out_pos = None if position_ids is None else torch.arange(total, device=position_ids.device,
                                                                 dtype=position_ids.dtype)[None]
        out_pos = _pos_skipping(self, out_pos, emb)
        return None, out_pos, out_mask, past_key_values, emb, out_labels


def _pos_skipping(lm, position_ids, emb):
    """`use_pos_skipping` (llava_arch.py:869-875, training only): position ids 0..L-1 with a random offset in front of
    and behind a random split point (long-context extension trick of the reference's trainer).  Same three draws from
    Python's `random`, in the same order."""
    if not (getattr(lm.config, "use_pos_skipping", False) and getattr(lm, "training", False)):
        return position_ids
    L = emb.size(1)
    position_ids = torch.arange(L, device=emb.device).unsqueeze(0)
    split_position = random.randint(0, L)
    left_add = random.randint(0, lm.config.pos_skipping_range)
    right_add = random.randint(left_add, lm.config.pos_skipping_range)
    position_ids[:, :split_position] += left_add
    position_ids[:, split_position:] += right_add
    return position_ids


def splice_into_text(lm, model, image_features: List[torch.Tensor], input_ids, position_ids, attention_mask,
                     past_key_values, labels):
    """Insert the visual token blocks at IMAGE_TOKEN_INDEX, truncate to tokenizer_model_max_length, pad, and build
    labels / mask / position ids (llava_arch.py:745-878).  Host-side orchestration of device copies."""
    _labels, _position_ids, _attention_mask = labels, position_ids, attention_mask
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids, dtype=torch.bool)
    else:
        attention_mask = attention_mask.bool()
    if position_ids is None:
        position_ids = torch.arange(0, input_ids.shape[1], dtype=torch.long, device=input_ids.device)
    if labels is None:
        labels = torch.full_like(input_ids, IGNORE_INDEX)
    ids_list = [i[m] for i, m in zip(input_ids, attention_mask)]
    lab_list = [l[m] for l, m in zip(labels, attention_mask)]

    new_embeds, new_labels = [], []
    img_i = 0
    for ids, lab in zip(ids_list, lab_list):
        img_pos = torch.where(ids == IMAGE_TOKEN_INDEX)[0].tolist()
        if not img_pos:
            new_embeds.append(model.embed_tokens(ids))
            new_labels.append(lab)
            img_i += 1
            continue
        cuts = [-1] + img_pos + [ids.shape[0]]
        text_ids = [ids[cuts[i] + 1:cuts[i + 1]] for i in range(len(cuts) - 1)]
        text_lab = [lab[cuts[i] + 1:cuts[i + 1]] for i in range(len(cuts) - 1)]
        text_emb = torch.split(model.embed_tokens(torch.cat(text_ids)), [t.shape[0] for t in text_ids], dim=0)
        pe, pl = [], []
        for i in range(len(img_pos) + 1):
            pe.append(text_emb[i])
            pl.append(text_lab[i])
            if i < len(img_pos):
                f = image_features[min(img_i, len(image_features) - 1)]
                img_i += 1
                pe.append(f.to(text_emb[i].dtype))
                pl.append(torch.full((f.shape[0],), IGNORE_INDEX, device=lab.device, dtype=lab.dtype))
        new_embeds.append(torch.cat(pe))
        new_labels.append(torch.cat(pl))

    max_tok = getattr(lm.config, "tokenizer_model_max_length", None)
    new_embeds = [x[:max_tok] for x in new_embeds]
    new_labels = [x[:max_tok] for x in new_labels]
    max_len = max(x.shape[0] for x in new_embeds)
    B = len(new_embeds)
    left = getattr(lm.config, "tokenizer_padding_side", "right") == "left"
    emb = torch.zeros((B, max_len, new_embeds[0].shape[1]), dtype=new_embeds[0].dtype, device=new_embeds[0].device)
    lab_pad = torch.full((B, max_len), IGNORE_INDEX, dtype=new_labels[0].dtype, device=new_labels[0].device)
    mask = torch.zeros((B, max_len), dtype=attention_mask.dtype, device=attention_mask.device)
    pos = torch.zeros((B, max_len), dtype=position_ids.dtype, device=position_ids.device)
    for i, (e, l) in enumerate(zip(new_embeds, new_labels)):
        n = e.shape[0]
        if n == 0:
            continue
        sl = slice(max_len - n, max_len) if left else slice(0, n)
        emb[i, sl] = e
        lab_pad[i, sl] = l
        mask[i, sl] = True
        pos[i, sl] = torch.arange(0, n, dtype=pos.dtype, device=pos.device)
    out_labels = None if _labels is None else lab_pad
    out_mask = None if _attention_mask is None else mask.to(dtype=_attention_mask.dtype)
    out_pos = _pos_skipping(lm, None if _position_ids is None else pos, emb)
    return None, out_pos, out_mask, past_key_values, emb, out_labels
