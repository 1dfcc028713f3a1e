"""The row widths tests/test_gpu_layernorm_forms.py launches, as literals: (form, D, residual row stride) for every form of the row
LayerNorm forward (csrc/elementwise.hip `ln_dispatch`).  tests/test_layernorm_forms_cpu.py holds the table to the C library's
`mavlm_layernorm_form` without a GPU - the function the dispatch itself switches on - so a change of the dispatch rule breaks
the literals there first and the coverage of the forms cannot rot silently.

Forms: 100 + c = `layernorm8_kernel<T, c>` (a wave per row, c chunks of 8 elements per lane), 200 = `layernorm8_block_kernel<T, 2>`
(a workgroup per row), 300 + v = `layernorm_kernel<T, v>` (the 4-element fallback, v float4 per lane), 0 = refused.  The widths
are the edges of each form: its narrowest and widest row, a single chunk, a partly filled last chunk row (D / 8 or D / 4 no
multiple of 64), and the widths of real configurations (896, 1024, 1152, 1536, 2048, 3584, 4096)."""

LN8, BLOCK, FALLBACK, REFUSED = 100, 200, 300, 0
MAX_D = 4096                                   # include/mavlm.h MAVLM_MAX_HIDDEN

# (form, D, residual row stride)
FORWARD_CASES = (
    [(LN8 + 1, d, d) for d in (8, 128, 504, 512)] +
    [(LN8 + 2, d, d) for d in (520, 896, 1024)] +
    [(LN8 + 4, d, d) for d in (1032, 1152, 1536, 2048)] +
    [(BLOCK, d, d) for d in (2056, 3584, 4088, 4096)] +
    [(FALLBACK + 1, d, d) for d in (4, 252)] +
    [(FALLBACK + 2, d, d) for d in (260, 508)] +
    [(FALLBACK + 4, d, d) for d in (516, 1020)] +
    [(FALLBACK + 8, d, d) for d in (1028, 2044)] +
    [(FALLBACK + 16, d, d) for d in (2052, 4092)] +
    # D % 8 == 0 over a residual whose row stride is 4 mod 8 (a [:, :D] view of a wider tensor): the fallback as well
    [(FALLBACK + 4, 1024, 1028), (FALLBACK + 16, 3584, 3588)]
)
REFUSED_CASES = [(REFUSED, 4100, 4100), (REFUSED, 4104, 4104), (REFUSED, 6, 6)]
ALL_FORMS = [LN8 + 1, LN8 + 2, LN8 + 4, BLOCK] + [FALLBACK + v for v in (1, 2, 4, 8, 16)] + [REFUSED]

# LayerNorm backward (csrc/backward.hip `launch_ln_bwd`): D -> float4 per lane NV; 4096 is the dynamic-LDS branch at its limit
BACKWARD_CASES = [(260, 2), (512, 2), (1536, 8), (2048, 8), (4096, 16)]
BACKWARD_REFUSED = 4100


def form_name(form):
    if form == REFUSED:
        return "refused"
    if form == BLOCK:
        return "block"
    return f"ln8-nc{form - LN8}" if form < BLOCK else f"fallback-nv{form - FALLBACK}"
