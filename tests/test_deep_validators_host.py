"""The validators of the deep-view family as one matrix: fr_deep_validate, fr_deep_ship_validate, fr_deepx_validate,
fr_deepx_ship_validate, fr_deep_julia_validate, fr_deepx_julia_validate and fr_deep_de_validate over the same inputs, with no
GPU.  Every cell pins the returned status and, where the message names the entry point, that name in fr_last_error.  The
expected cells were recorded from the library as it stood before the validators were folded onto one rule table
(fr_deep.c: kRules, validate_params, resolve_view); a cell that changes is a change of behaviour.  A second matrix does the
same for what the six *_reference_orbit(s) functions ask before they iterate (orbit_request), there with the whole text."""
import ctypes as C
import math

import pytest

W = H = 8

# validator -> (library symbol, the entry point its messages name, fractal type, extended view)
VALIDATORS = {
    "deep": ("fr_deep_validate", "fr_render_deep", 0, False),
    "deep_ship": ("fr_deep_ship_validate", "fr_render_deep_ship", 2, False),
    "deepx": ("fr_deepx_validate", "fr_render_deepx", 0, True),
    "deepx_ship": ("fr_deepx_ship_validate", "fr_render_deepx_ship", 2, True),
    "deep_julia": ("fr_deep_julia_validate", "fr_render_deep_julia", 1, False),
    "deepx_julia": ("fr_deepx_julia_validate", "fr_render_deepx_julia", 1, True),
    "deep_de": ("fr_deep_de_validate", "fr_render_deep", 0, False),
}
ORDER = list(VALIDATORS)

# the zoom at both ends of its range and just outside: p->zoom in [1e-290, 1e3], the view's string in [1e-1000, 1e3]
ZOOMS = {"lo": (1e-290, "1e-1000"), "hi": (1e3, "1e3"), "below": (math.nextafter(1e-290, 0.0), "9.999999999e-1001"),
         "above": (math.nextafter(1e3, math.inf), "1000.0000001")}
BLA = {"DEEP_BLA": 0x2, "DEEPX_BLA": 0x4, "DEEP_SHIP_BLA": 0x8, "DEEPX_SHIP_BLA": 0x10, "DEEP_JULIA_BLA": 0x20,
       "DEEPX_JULIA_BLA": 0x40}

# case -> what it changes: fields of fr_params by name; "view": fields of the view; "zoom": a key of ZOOMS; "wrong_type": a
# fractal type that is not the validator's
CASES = {
    "ok": {},
    **{"flag_" + k: dict(flags=v) for k, v in BLA.items()},
    "wrong_type": dict(wrong_type=True),
    "precision_f32": dict(precision=0),
    "orbit_trap": dict(orbit_trap_enabled=1),
    "stripes": dict(stripe_enabled=1),
    "stripes_interior_2": dict(stripe_enabled=1, interior_style=2),
    "interior_2": dict(interior_style=2),
    "interior_3": dict(interior_style=3),
    **{"zoom_" + k: dict(zoom=k) for k in ZOOMS},
    "bailout_0": dict(bailout=0.0),
    "bailout_65536": dict(bailout=65536.0),
    "bailout_65537": dict(bailout=65537.0),
    "bailout_1e6": dict(bailout=1e6),
    "reserved_1": dict(view=dict(reserved=1)),
    **{"frac_bits_%d" % b: dict(view=dict(frac_bits=b)) for b in (0, 127, 128, 4096, 4097)},
    "cx_null": dict(view=dict(center_x=None)),
    "cy_null": dict(view=dict(center_y=None)),
    "cx_malformed": dict(view=dict(center_x=b"1e")),
    "cy_empty": dict(view=dict(center_y=b"")),
    "cx_2pow32": dict(view=dict(center_x=b"4294967296")),
    "cy_minus_2pow32": dict(view=dict(center_y=b"-4294967296")),
    "cx_below_2pow32": dict(bailout=65536.0, view=dict(center_x=b"4294967295.999")),
    "julia_c_nan": dict(julia_c_real=float("nan")),
    "julia_c_inf": dict(julia_c_imag=float("inf")),
    "julia_c_2pow32": dict(julia_c_real=4294967296.0),
    "julia_c_below_2pow32": dict(julia_c_imag=-4294967295.0),
    "centre_outside_bailout": dict(view=dict(center_x=b"-3", center_y=b"3")),
    "centre_on_bailout": dict(view=dict(center_x=b"4", center_y=b"0")),
    # two rules at once: the first failing check decides
    "two_wrong_type_and_bailout_0": dict(wrong_type=True, bailout=0.0),              # the type comes first: unsupported
    "two_bailout_0_and_orbit_trap": dict(bailout=0.0, orbit_trap_enabled=1),         # the bailout comes first: invalid
    "two_foreign_flags_and_reserved": dict(flags=0x2 | 0x20, view=dict(reserved=1)),  # the flags come first: unsupported
    # p->zoom comes before the whole-orbit rule (invalid); a view's zoom string is read after it (fr_deepx_validate: unsupported;
    # the ship accepts interior_style 2 without stripes and Julia ignores it, so there the zoom decides)
    "two_zoom_below_and_interior_2": dict(zoom="below", interior_style=2),
}

# One letter per validator, in ORDER: o = FR_OK, e = FR_ERR_INVALID_ARG, u = FR_ERR_UNSUPPORTED; a capital: the message names the
# validator's entry point
EXPECT = {
    "ok": "ooooooo",
    "flag_DEEP_BLA": "oUUUUUo",
    "flag_DEEPX_BLA": "oUoUUUo",
    "flag_DEEP_SHIP_BLA": "oooUUUo",
    "flag_DEEPX_SHIP_BLA": "ooooUUo",
    "flag_DEEP_JULIA_BLA": "UUUUoUU",
    "flag_DEEPX_JULIA_BLA": "UUUUUoU",
    "wrong_type": "UUUUUUU",
    "precision_f32": "UUUUUUU",
    "orbit_trap": "UUUUooU",
    "stripes": "UoUoooU",
    "stripes_interior_2": "UUUUooU",
    "interior_2": "UoUoooU",
    "interior_3": "oUoUooo",
    "zoom_lo": "ooooooo",
    "zoom_hi": "ooooooo",
    "zoom_below": "eeeeeee",
    "zoom_above": "eeeeeee",
    "bailout_0": "eeeeeee",
    "bailout_65536": "ooooooo",
    "bailout_65537": "eeeeeee",
    "bailout_1e6": "eeeeeee",
    "reserved_1": "eeeeeee",
    "frac_bits_0": "ooooooo",
    "frac_bits_127": "eeeeeee",
    "frac_bits_128": "ooooooo",
    "frac_bits_4096": "ooooooo",
    "frac_bits_4097": "eeeeeee",
    "cx_null": "eeeeeee",
    "cy_null": "eeeeeee",
    "cx_malformed": "eeeeeee",
    "cy_empty": "eeeeeee",
    "cx_2pow32": "eeeeeee",
    "cy_minus_2pow32": "eeeeeee",
    "cx_below_2pow32": "ooooeeo",
    "julia_c_nan": "eeeeeee",
    "julia_c_inf": "eeeeeee",
    "julia_c_2pow32": "ooooeeo",
    "julia_c_below_2pow32": "ooooooo",
    "centre_outside_bailout": "ooooeeo",
    "centre_on_bailout": "ooooooo",
    "two_wrong_type_and_bailout_0": "UUUUUUU",
    "two_bailout_0_and_orbit_trap": "eeeeeee",
    "two_foreign_flags_and_reserved": "UUUUUUU",
    "two_zoom_below_and_interior_2": "eeUeeee",
}
STATUS = {"o": 0, "e": -1, "u": -4}


def observe(fr, validator, case):
    """(status, message) of one cell; the message is only meaningful with a status other than FR_OK"""
    K, L = fr._capi, fr.lib()
    symbol, _, fractal, ext = VALIDATORS[validator]
    change = dict(CASES[case])
    p = fr.FractalState(max_iterations=64, zoom=1e-30).to_params(fr.FractalType(fractal), fr.Precision.F64, False)
    view = dict(center_x=b"0", center_y=b"0", frac_bits=0, reserved=0)
    zoom_s = b"1e-400"
    view.update(change.pop("view", {}))
    if change.pop("wrong_type", False):
        p.fractal_type = {0: 1, 1: 0, 2: 0}[fractal]
    z = change.pop("zoom", None)
    if z is not None:
        p.zoom, zoom_s = ZOOMS[z][0], ZOOMS[z][1].encode()
    for k, val in change.items():
        assert hasattr(p, k), k
        setattr(p, k, val)
    v = (K.fr_deepx_view(view["center_x"], view["center_y"], zoom_s, view["frac_bits"], view["reserved"]) if ext else
         K.fr_deep_view(view["center_x"], view["center_y"], view["frac_bits"], view["reserved"]))
    fn = getattr(L, symbol)
    fn.restype = C.c_int
    if validator == "deep_de":
        e = K.fr_deep_de(None, None, 0, 1.8)
        st = fn(C.byref(p), C.byref(v), C.byref(e), W, H)
    else:
        st = fn(C.byref(p), C.byref(v), W, H)
    return st, L.fr_last_error().decode("utf-8", "replace")


def names_entry(validator, message):
    who = VALIDATORS[validator][1]
    return message.startswith(who + " ") or message.startswith(who + ":")


def test_the_matrix_is_complete():
    assert set(EXPECT) == set(CASES) and all(len(row) == len(ORDER) for row in EXPECT.values())


@pytest.mark.parametrize("validator", ORDER)
@pytest.mark.parametrize("case", list(CASES))
def test_validator_matrix(fr, case, validator):
    want = EXPECT[case][ORDER.index(validator)]
    st, msg = observe(fr, validator, case)
    assert st == STATUS[want.lower()], (case, validator, st, msg)
    if want.isupper():
        assert names_entry(validator, msg), (case, validator, msg)
    elif st != 0:
        assert not names_entry(validator, msg), (case, validator, msg)


# ---- the six reference-orbit entry points: what they ask before they iterate --------------------------------------------------
# function -> (extended view, Julia); every call asks for 8 updates
ORBITS = {
    "fr_deep_reference_orbit": (False, False),
    "fr_deep_ship_reference_orbit": (False, False),
    "fr_deepx_reference_orbit": (True, False),
    "fr_deepx_ship_reference_orbit": (True, False),
    "fr_deep_julia_reference_orbits": (False, True),
    "fr_deepx_julia_reference_orbits": (True, True),
}
ORBIT_ORDER = list(ORBITS)

# case -> what it changes: view=None, out=None (the first out pointer), len=None (the last one), max_iter, zoom (the fp64 entries'
# double), zoom_s (the extended views' string), bailout, c_re, or fields of the view
ORBIT_CASES = {
    "ok": {},
    "view_null": dict(view=None),
    "out_null": dict(out=None),
    "len_null": dict(len=None),
    "max_iter_0": dict(max_iter=0),
    "max_iter_above": dict(max_iter=(1 << 24) + 1),
    "zoom_below": dict(zoom=1e-291),
    "zoom_string_null": dict(zoom_s=None),
    "zoom_string_below": dict(zoom_s=b"1e-1001"),
    "zoom_string_malformed": dict(zoom_s=b"z"),
    "bailout_0": dict(bailout=0.0),
    "bailout_above": dict(bailout=65537.0),
    "c_nan": dict(c_re=float("nan")),
    "c_2pow32": dict(c_re=4294967296.0),
    "reserved_1": dict(reserved=1),
    "frac_bits_127": dict(frac_bits=127),
    "cx_null": dict(center_x=None),
    "cy_malformed": dict(center_y=b"1e"),
    "cx_2pow32": dict(center_x=b"4294967296"),
    "centre_outside_bailout": dict(center_x=b"-3", center_y=b"3"),
    # two at once: the first failing check decides the text
    "two_view_null_and_bailout_0": dict(view=None, bailout=0.0),
    "two_view_null_and_zoom_below": dict(view=None, zoom=1e-291),
    "two_view_null_and_max_iter_0": dict(view=None, max_iter=0),
    "two_out_null_and_view_null": dict(out=None, view=None),
    "two_c_nan_and_reserved_1": dict(c_re=float("nan"), reserved=1),
}


def observe_orbit(fr, name, case):
    """(status, message) of one call; the message is only meaningful with a status other than FR_OK"""
    import numpy as np
    K, L = fr._capi, fr.lib()
    ext, julia = ORBITS[name]
    ch = dict(ORBIT_CASES[case])
    fields = dict(center_x=b"0", center_y=b"0", frac_bits=0, reserved=0)
    fields.update({k: ch.pop(k) for k in list(ch) if k in fields})
    zoom_s = ch.pop("zoom_s", b"1e-400")
    if "view" in ch:
        vp = None
    elif ext:
        vp = C.byref(K.fr_deepx_view(fields["center_x"], fields["center_y"], zoom_s, fields["frac_bits"], fields["reserved"]))
    else:
        vp = C.byref(K.fr_deep_view(fields["center_x"], fields["center_y"], fields["frac_bits"], fields["reserved"]))
    n = ch.get("max_iter", 8)
    bufs = [np.zeros((10, 2)) for _ in range(2)] + [np.zeros(10, np.int32) for _ in range(2)]
    lens = [C.c_int32(), C.c_int32()]
    first = None if "out" in ch else bufs[0].ctypes.data
    last = None if "len" in ch else C.byref(lens[1])
    zoom = (C.c_double(ch.get("zoom", 1e-30)),) if not ext else ()
    bail = C.c_float(ch.get("bailout", 4.0))
    cc = (C.c_double(ch.get("c_re", -0.12)), C.c_double(0.74)) if julia else ()
    exp = lambda i: (C.c_void_p(bufs[2 + i].ctypes.data),) if ext else ()
    if julia:
        outs = (C.c_void_p(first),) + exp(0) + (C.byref(lens[0]), C.c_void_p(bufs[1].ctypes.data)) + exp(1) + (last,)
    else:
        outs = (C.c_void_p(first),) + exp(0) + (last,)
    st = getattr(L, name)(vp, *cc, *zoom, n, bail, *outs)
    return st, L.fr_last_error().decode("utf-8", "replace")


# every refusal here is FR_ERR_INVALID_ARG with one of these texts ({who}: the function called), recorded like EXPECT above
MSG = {
    "view": "deep view is NULL",
    "out": "{who}: out is NULL",
    "n0": "max_iterations 0 outside [1, 2^24]",
    "n+": "max_iterations 16777217 outside [1, 2^24]",
    "zoom": "deep zoom 1e-291 outside [1e-290, 1e3]",
    "zs_null": "deep zoom string is NULL",
    "zs_range": "deep zoom outside [1e-1000, 1e3]",
    "zs_form": "deep zoom is not [+-]digits[.digits][(e|E)[+-]digits] of at most 4096 characters",
    "bail": "deep bailout must be finite, > 0 and <= 2^16",
    "c": "deep Julia views need a finite c with |c_re|, |c_im| < 2^32",
    "res": "fr_deep_view.reserved must be 0",
    "resx": "fr_deepx_view.reserved must be 0",
    "bits": "frac_bits 127 outside {0} U [128, 4096]",
    "cx_null": "deep view centre string is NULL",
    "cy_form": "deep view center_y is not [+-]digits[.digits][(e|E)[+-]digits] of at most 4096 characters",
    "cx_big": "deep view center_x: |centre| must be < 2^32",
    "outside": "deep Julia view: the centre lies outside the bailout radius (|centre|^2 > bailout^2)",
}
# a key of MSG per function, in ORBIT_ORDER (deep, deep_ship, deepx, deepx_ship, deep_julia, deepx_julia); None: FR_OK
ORBIT_EXPECT = {
    "ok": [None] * 6,
    "view_null": ["view"] * 6,
    "out_null": ["out"] * 6,
    "len_null": ["out"] * 6,
    "max_iter_0": ["n0"] * 6,
    "max_iter_above": ["n+"] * 6,
    "zoom_below": ["zoom", "zoom", None, None, "zoom", None],
    "zoom_string_null": [None, None, "zs_null", "zs_null", None, "zs_null"],
    "zoom_string_below": [None, None, "zs_range", "zs_range", None, "zs_range"],
    "zoom_string_malformed": [None, None, "zs_form", "zs_form", None, "zs_form"],
    "bailout_0": ["bail"] * 6,
    "bailout_above": ["bail"] * 6,
    "c_nan": [None, None, None, None, "c", "c"],
    "c_2pow32": [None, None, None, None, "c", "c"],
    "reserved_1": ["res", "res", "resx", "resx", "res", "resx"],
    "frac_bits_127": ["bits"] * 6,
    "cx_null": ["cx_null"] * 6,
    "cy_malformed": ["cy_form"] * 6,
    "cx_2pow32": ["cx_big"] * 6,
    "centre_outside_bailout": [None, None, None, None, "outside", "outside"],
    "two_view_null_and_bailout_0": ["bail"] * 6,                 # the bailout comes before the view
    "two_view_null_and_zoom_below": ["zoom", "zoom", "view", "view", "zoom", "view"],   # a double zoom too; a string is the view's
    "two_view_null_and_max_iter_0": ["n0"] * 6,
    "two_out_null_and_view_null": ["out"] * 6,
    "two_c_nan_and_reserved_1": ["res", "res", "resx", "resx", "c", "c"],
}


def test_the_orbit_matrix_is_complete():
    assert set(ORBIT_EXPECT) == set(ORBIT_CASES) and all(len(row) == len(ORBIT_ORDER) for row in ORBIT_EXPECT.values())


@pytest.mark.parametrize("name", ORBIT_ORDER)
@pytest.mark.parametrize("case", list(ORBIT_CASES))
def test_reference_orbit_requests(fr, case, name):
    want = ORBIT_EXPECT[case][ORBIT_ORDER.index(name)]
    st, msg = observe_orbit(fr, name, case)
    if want is None:
        assert st == 0, (case, name, st, msg)
    else:
        assert (st, msg) == (-1, MSG[want].replace("{who}", name)), (case, name)
