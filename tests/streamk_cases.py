"""The schedules of the attention forward that tests/test_gpu_streamk_levels.py launches, as literals: one table of
(kernel, hooks, shape) -> (whole rounds, level list), shared with the CPU mirror test (tests/test_plan_mirror_cpu.py), which holds
the C library and the oracle to it without a GPU.  A change of the plan rule breaks the literals there first, so the coverage
of the cut levels cannot rot silently.

Kernels: "w8" / "w4" = attn_fwd3_kernel (head_dim 128) with 8- / 4-wave workgroups (`mavlm_set_attention_streamk_waves`), units of
256 / 128 queries on G = 256 / 512 workgroups; "wide" = attn_fwd_hd2_kernel (head_dim 448), 128-query units, G = 256.  All under
`mavlm_set_attention_streamk_min_tiles(1)`.  A level is (k, first unit, units): its units are cut into 2^k key ranges."""

MIN_TILES = 1
WAVES = {"w8": 8, "w4": 4, "wide": 0}
S_NARROW = 64 * 33 + 5        # 34 key tiles of 64, the last ragged: not divisible by any 2^k
S_WIDE = 32 * 33 + 5          # the same for the 32-key tiles of the wide kernel
S_EMPTY = 256                 # 4 (8) key tiles: a 32-way cut has empty pieces

# (kernel, R, S, H, G, whole rounds, levels)
STREAMK_CASES = [
    ("w8", 65792, S_NARROW, 1, 256, 1, [(5, 256, 1)]),                 # a one-unit level
    ("w8", 8448, S_NARROW, 8, 256, 1, [(5, 256, 8)]),
    ("w8", 8704, S_NARROW, 8, 256, 1, [(4, 256, 16)]),
    ("w8", 9213, S_NARROW, 8, 256, 1, [(3, 256, 32)]),                 # ragged last query block
    ("w8", 10240, S_NARROW, 8, 256, 1, [(2, 256, 64)]),
    ("w8", 12288, S_NARROW, 8, 256, 1, [(1, 256, 128)]),
    ("w8", 62199, S_NARROW, 2, 256, 1, [(1, 256, 128), (2, 384, 64), (3, 448, 32), (5, 480, 6)]),   # four levels, a short last one
    ("w8", 62194, S_NARROW, 2, 256, 1, [(1, 256, 128), (2, 384, 64), (3, 448, 32), (5, 480, 6)]),   # ... five rows fewer
    ("w8", 20729, S_NARROW, 8, 256, 2, [(1, 512, 128), (5, 640, 8)]),
    ("w8", 43776, S_NARROW, 3, 256, 2, [(5, 512, 1)]),
    ("w8", 8448, S_EMPTY, 8, 256, 1, [(5, 256, 8)]),
    ("w4", 8320, S_NARROW, 8, 512, 1, [(5, 512, 8)]),
    ("w4", 8704, S_NARROW, 8, 512, 1, [(4, 512, 32)]),
    ("w4", 9216, S_NARROW, 8, 512, 1, [(3, 512, 64)]),
    ("w4", 10240, S_NARROW, 8, 512, 1, [(2, 512, 128)]),
    ("w4", 12155, S_NARROW, 8, 512, 1, [(2, 512, 128), (3, 640, 64), (4, 704, 32), (5, 736, 16), (5, 752, 8)]),   # five levels
    ("w4", 18549, S_NARROW, 8, 512, 2, [(2, 1024, 128), (5, 1152, 8)]),
    ("w4", 8320, S_EMPTY, 8, 512, 1, [(5, 512, 8)]),
    ("wide", 5120, S_WIDE, 8, 256, 1, [(2, 256, 64)]),
    ("wide", 7168, S_WIDE, 8, 256, 1, [(1, 256, 128), (2, 384, 64)]),
    ("wide", 7552, S_WIDE, 8, 256, 1, [(1, 256, 128), (2, 384, 64), (4, 448, 16), (5, 464, 8)]),
    ("wide", 7547, S_WIDE, 8, 256, 1, [(1, 256, 128), (2, 384, 64), (4, 448, 16), (5, 464, 8)]),   # ... five rows fewer
    ("wide", 7680, S_WIDE, 8, 256, 1, [(1, 256, 128), (2, 384, 64), (3, 448, 32)]),
    ("wide", 12416, S_WIDE, 8, 256, 3, [(5, 768, 8)]),
    ("wide", 12416, S_EMPTY, 8, 256, 3, [(5, 768, 8)]),
]

# Row batches (`mavlm_attention_batch`): H counts the (video, head) pairs of all nb videos; the automatic workgroup shape
# (8 waves at head_dim 128).  (kernel, nb, R per video, S, H, G, whole rounds, levels)
BATCH_CASES = [
    ("w8", 2, 6267, S_NARROW, 16, 256, 1, [(1, 256, 128), (4, 384, 16)]),
    ("wide", 2, 3771, S_WIDE, 16, 256, 1, [(1, 256, 128), (2, 384, 64), (3, 448, 32)]),
    ("wide", 3, 2389, S_WIDE, 24, 256, 1, [(1, 256, 128), (2, 384, 64), (5, 448, 8)]),
]

# Split-KV of the small grids, default hooks: (R, S, H, planes at head_dim 128 | None, planes at head_dim 448 | None); every plane
# count at least once with a ragged last key tile and a last plane that holds fewer tiles than the others
SPLIT_CASES = [
    (300, 1061, 2, 2, None),
    (300, 1100, 2, None, 2),
    (392, 1980, 8, 3, 3),
    (392, 2117, 8, 4, 4),
    (256, 3000, 8, 5, 5),
    (392, 3100, 8, 6, 6),
    (640, 6272, 8, None, 6),
    (392, 3950, 8, 7, 7),
    (392, 4000, 8, 7, 7),
    (200, 6272, 8, 8, 7),
    (128, 4096, 3, 8, None),
    (392, 4100, 8, 8, 7),
]


def cases_of(kernel):
    return [c for c in STREAMK_CASES if c[0] == kernel]


def case_id(c):
    return f"{c[0]}-R{c[1]}-S{c[2]}-H{c[3]}"
