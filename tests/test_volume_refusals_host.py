"""CPU tier: the volume entries (metrics, MS-SSIM, mask scores, components, preprocessing) refuse a bad descriptor with the return code and
the words an earlier build of the library gives, also where a descriptor has two faults at once and the order of the checks decides which
one is reported.  DM3D_PARENT_LIB names that earlier libdm3d_hip.so; without it the test skips.  Nothing is launched and nothing is built."""
import ctypes as C
import os

import pytest

import test_components_host as cc
import test_mask_host as mk
import test_metrics_host as mt
import test_msssim_host as ms
import test_resample_host as rs

PARENT = os.environ.get("DM3D_PARENT_LIB")
A = 0x10000


def _rows():
    """(entry point, descriptor builder, override or None for the NULL call): every row of the five BAD tables, then the double faults."""
    rows = []
    for entries, override, _ in mt.BAD:
        rows += [(e, mt._desc, override) for e in entries]
    rows += [("dm3d_ms_ssim", ms._desc, override) for override, _ in ms.BAD]
    for mod in (mk, cc):
        for entries, override, _ in mod.BAD:
            rows += [(mod.ENTRIES[e], mod._desc, override) for e in entries]
    rows += [(rs.ENTRY[short], lambda lib, short=short, **o: rs._desc(lib, short, **o), override) for short, override, _ in rs.BAD]
    both = dict(x0c=-1, y0c=-1)                                     # a bad x window with a bad y window
    rows += [(e, mt._desc, both) for e in mt.ENTRIES[:2]] + [("dm3d_ms_ssim", ms._desc, both)]
    rows += [(mk.ENTRIES[e], mk._desc, both) for e in ("mask_overlap", "surface_distance")]
    for mod in (mk, cc):                                            # a bad extent with a bad nc, a bad nc with a bad window, a bad threshold last
        for override in (dict(d=513, nc=0), dict(w=0, nc=0), dict(batch=0, h=513), dict(nc=0, x0c=-1), dict(batch=32768, x0c=2),
                         dict(x0c=-1, threshold=float("nan")), dict(d=513, threshold=float("inf"))):
            rows += [(name, mod._desc, override) for name in mod.ENTRIES.values()]
    rows += [("dm3d_ms_ssim", ms._desc, dict(nc=0, x0c=-1)), ("dm3d_ms_ssim", ms._desc, dict(d=0, y0c=2))]
    rows += [(e, mt._desc, dict(nc=0, x0c=1)) for e in mt.ENTRIES]
    # a misaligned buffer with a short *_elems
    rows += [("dm3d_pair_stats", mt._desc, dict(partials=A + 4, partials_elems=1)), ("dm3d_ssim", mt._desc, dict(partials=A + 4, partials_elems=1)),
             ("dm3d_ms_ssim", ms._desc, dict(partials=A + 4, partials_elems=1)), ("dm3d_edt", mk._desc, dict(map=A + 2, masks_elems=1)),
             ("dm3d_surface_distance", mk._desc, dict(work=A + 2, work_elems=1)), ("dm3d_surface_distance", mk._desc, dict(out=A + 4, masks_elems=1)),
             ("dm3d_components", cc._desc, dict(work=A + 4, work_elems=1)), ("dm3d_component_filter", cc._desc, dict(out=A + 0x100001, work_elems=1)),
             ("dm3d_components", cc._desc, dict(x=A + 2, nc=3))]
    # the prefilter's grid limit (the three passes share one check), alone and behind a bad extent
    spline = lambda lib, **o: rs._desc(lib, "spline_filter", **o)
    rows += [("dm3d_spline_filter", spline, dict(volumes=2 ** 31 - 1, d=512, h=512, w=1)), ("dm3d_spline_filter", spline, dict(volumes=2 ** 31 - 1, d=1, h=1, w=512)),
             ("dm3d_spline_filter", spline, dict(volumes=2 ** 31 - 1, d=512, h=1, w=512)), ("dm3d_spline_filter", spline, dict(volumes=2 ** 31 - 1, d=513, h=512)),
             ("dm3d_spline_filter", spline, dict(coeff=A + 4, volumes=0))]
    for name, make in [(e, mt._desc) for e in mt.ENTRIES] + [("dm3d_ms_ssim", ms._desc)] + [(n, mk._desc) for n in mk.ENTRIES.values()] + [
            (n, cc._desc) for n in cc.ENTRIES.values()] + [(n, None) for n in rs.ENTRY.values()]:
        rows.append((name, make, None))
    return rows


@pytest.mark.skipif(not PARENT, reason="DM3D_PARENT_LIB (an earlier build of libdm3d_hip.so to compare against) is not set")
def test_refusals_equal_the_parent_librarys(built_library):
    from dm3d_amd import _lib
    libs = [C.CDLL(built_library), C.CDLL(PARENT)]
    assert built_library != PARENT and os.path.exists(PARENT)
    for lib in libs:
        for name, (res, args) in _lib.SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    rows, failures = _rows(), []
    for name, make, override in rows:
        got = []
        for lib in libs:
            lib.dm3d_fill(None, 0, 0.0, None)            # leaves a known message behind
            rc = getattr(lib, name)(None if override is None else C.byref(make(_lib, **override)), None)
            got.append((rc, (lib.dm3d_last_error() or b"").decode()))
        print(f"{'same' if got[0] == got[1] else 'DIFFERENT'} {name}({override}): {got[0]}" + ("" if got[0] == got[1] else f" parent {got[1]}"))
        if got[0] != got[1] or got[0][0] != -1:
            failures.append(f"{name}({override}): {got[0]} parent {got[1]}")
    print(f"{len(rows)} refusals compared, {len(failures)} differ or are no refusal")
    assert len(rows) > 300 and not failures, "\n".join(failures)
