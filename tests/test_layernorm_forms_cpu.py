"""CPU: the table of tests/layernorm_cases.py against the C library's `mavlm_layernorm_form` - the function `ln_dispatch`
(csrc/elementwise.hip) switches on.  Every width of the table takes the form the table claims, every form has at least one
width, and the form boundaries sit where the table's edge widths assume them."""
import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
import layernorm_cases as L


def test_every_table_width_takes_its_form():
    lib = capi.lib()
    for form, d, ldr in L.FORWARD_CASES + L.REFUSED_CASES:
        assert lib.mavlm_layernorm_form(d, ldr) == form, (L.form_name(form), d, ldr)
    for form, d, ldr in L.FORWARD_CASES:
        if ldr == d and d % 8 == 0:
            assert lib.mavlm_layernorm_form(d, 0) == form, (d, "no residual")      # stride 0: the call without a residual


def test_every_form_has_a_case():
    seen = {form for form, _, _ in L.FORWARD_CASES + L.REFUSED_CASES}
    assert seen == set(L.ALL_FORMS)
    by_form = {}
    for form, d, ldr in L.FORWARD_CASES:
        by_form.setdefault(form, []).append(d)
    assert all(len(v) >= 2 for v in by_form.values()), by_form               # both edges of every launched form


def test_form_boundaries():
    """The whole admitted range, not only the table: the form is a step function of D with the steps the kernels' chunk counts
    give (64 lanes x 8 or 4 elements x chunks per lane), and nothing above MAX_D or off the 4-element grid is launched."""
    f = capi.lib().mavlm_layernorm_form
    for d in range(1, L.MAX_D + 64):
        for ldr in (0, d, d + 4, d + 2):
            got = f(d, ldr)
            if d % 4 or ldr % 4 or d > L.MAX_D:
                want = L.REFUSED
            elif d % 8 == 0 and ldr % 8 == 0:
                want = L.LN8 + 1 if d <= 512 else L.LN8 + 2 if d <= 1024 else L.LN8 + 4 if d <= 2048 else L.BLOCK
            else:
                want = L.FALLBACK + next(v for v in (1, 2, 4, 8, 16) if d <= 256 * v)
            assert got == want, (d, ldr, got, want)
    assert f(0, 0) == f(-8, 0) == f(8, -8) == L.REFUSED
    assert L.MAX_D == 4096 and f(L.MAX_D, L.MAX_D) == L.BLOCK and f(L.MAX_D, L.MAX_D + 4) == L.FALLBACK + 16
