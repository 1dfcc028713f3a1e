"""The launches of tests/test_gpu_fused_layernorm.py, as literals: the fused dense + residual + LayerNorm GEMM (EPI_LN of
csrc/gemm256.hip, and of csrc/gemm128.hip under `mavlm_set_gemm_tile(129)`).  tests/test_fused_ln_cases_cpu.py holds the table to the
C library's `mavlm_linear_ln_ws_bytes` without a GPU - the function the operator itself asks whether a shape takes the fused form -
and asserts what the table covers, so a change of the admission rule breaks the literals there first.

A case is (M, N, K, mode, fused hook, gemm_tile, gemm_rows, eps):
  fused hook  `mavlm_set_fused_layernorm`: 1 = the product's rule (N <= 1024: up to 4 partners per row block), 2 = the test hook
              (up to 16 partners: thread t polls granules t, t + 512, ... of the (partners - 1) x 2 x height others)
  gemm_tile   `mavlm_set_gemm_tile`: 0 = the 256-column-tile kernel of gemm256.hip, 129 = the 128-row form of gemm128.hip
  gemm_rows   `mavlm_set_gemm_rows`: the height of the workgroup tile, 224 or 256 (gemm_tile 129 has one height, 128: 256 is set)

The kernel is taken where ceil(M / 256) x (N / 256) >= 192: WIDTHS holds the smallest M per width, and the shapes are the smallest
that qualify.  N = 3584 (14 partners) stays with tests/test_gpu_ov7b_width.py."""

#        N: (partners = N / 256, fused hook, smallest M that takes the fused form)
WIDTHS = {256: (1, 1, 48897), 512: (2, 1, 24321), 768: (3, 1, 16129), 1024: (4, 1, 12033),
          1280: (5, 2, 9729), 2048: (8, 2, 5889), 4096: (16, 2, 2817)}
PARTNERS = (1, 2, 3, 4, 5, 8, 16)
HEIGHTS = (224, 256)

CASES = [
    # N = 1024, both heights: M mod height = 0, 1, height - 1 for both (12 544 = 49 x 256 = 56 x 224), and 12 288 / 12 289 for 256
    (12288, 1024, 1024, "bf16", 1, 0, 256, 1e-12),
    (12289, 1024, 1024, "bf16", 1, 0, 256, 1e-12),
    (12543, 1024, 1024, "bf16", 1, 0, 256, 1e-12),
    (12544, 1024, 1024, "bf16", 1, 0, 256, 1e-12),
    (12545, 1024, 1024, "bf16", 1, 0, 256, 1e-12),
    (12288, 1024, 1024, "bf16", 1, 0, 224, 1e-12),
    (12289, 1024, 1024, "bf16", 1, 0, 224, 1e-12),
    (12543, 1024, 1024, "bf16", 1, 0, 224, 1e-12),
    (12544, 1024, 1024, "bf16", 1, 0, 224, 1e-12),
    (12545, 1024, 1024, "bf16", 1, 0, 224, 1e-12),
    (12543, 1024, 1024, "fp16", 1, 0, 256, 1e-12),
    (12545, 1024, 1024, "fp16", 1, 0, 256, 1e-12),
    (12545, 1024, 1024, "fp16", 1, 0, 224, 1e-12),
    # a single K tile, and three
    (12545, 1024, 64, "bf16", 1, 0, 256, 1e-12),
    (12545, 1024, 64, "bf16", 1, 0, 224, 1e-12),
    (12289, 1024, 192, "fp16", 1, 0, 256, 1e-12),
    # eps 1e-5
    (12545, 1024, 1024, "bf16", 1, 0, 224, 1e-5),
    (12544, 1024, 64, "fp16", 1, 0, 256, 1e-5),
    # more tiles than one round of 256 workgroups: 66 x 4 = 264 (256 rows), 75 x 4 = 300 (224 rows); row blocks straddle rounds
    (16641, 1024, 64, "bf16", 1, 0, 256, 1e-12),
    (16641, 1024, 192, "fp16", 1, 0, 224, 1e-12),
    # the 128-row form (row blocks of 128 rows; 12 545 = 98 x 128 + 1)
    (12545, 1024, 1024, "bf16", 1, 129, 256, 1e-12),
    (12543, 1024, 1024, "fp16", 1, 129, 256, 1e-12),
    (24321, 512, 64, "bf16", 1, 129, 256, 1e-12),
    # N = 256: no partner
    (48897, 256, 64, "bf16", 1, 0, 256, 1e-12),
    (48897, 256, 64, "fp16", 1, 0, 224, 1e-12),
    (49151, 256, 192, "bf16", 1, 0, 224, 1e-12),
    # N = 512: 2 partners
    (24321, 512, 64, "bf16", 1, 0, 256, 1e-12),
    (24321, 512, 192, "bf16", 1, 0, 224, 1e-12),
    (24575, 512, 64, "fp16", 1, 0, 256, 1e-12),
    # N = 768: 3
    (16129, 768, 64, "bf16", 1, 0, 256, 1e-12),
    (16129, 768, 64, "fp16", 1, 0, 224, 1e-12),
    (16351, 768, 192, "bf16", 1, 0, 224, 1e-12),
    # N = 1280: 5, the first width only the test hook admits
    (9729, 1280, 64, "bf16", 2, 0, 256, 1e-12),
    (9729, 1280, 64, "fp16", 2, 0, 224, 1e-12),
    (9983, 1280, 192, "bf16", 2, 0, 256, 1e-12),
    # N = 2048: 8
    (5889, 2048, 64, "bf16", 2, 0, 256, 1e-12),
    (5889, 2048, 64, "fp16", 2, 0, 224, 1e-12),
    (6047, 2048, 192, "bf16", 2, 0, 224, 1e-12),
    # N = 4096: 16, the widest row
    (2817, 4096, 64, "bf16", 2, 0, 256, 1e-12),
    (2817, 4096, 64, "fp16", 2, 0, 224, 1e-12),
    (3071, 4096, 192, "bf16", 2, 0, 256, 1e-12),
    (2817, 4096, 1024, "bf16", 2, 0, 224, 1e-5),
]


def case_id(case):
    M, N, K, mode, hook, tile, rows, eps = case
    return f"M{M}-N{N}-K{K}-{mode}-" + ("tile129" if tile == 129 else f"rows{rows}") + ("" if eps == 1e-12 else f"-eps{eps:g}")
