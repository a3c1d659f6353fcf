"""CPU tests of the C entries of the behaviour map's segmentation (include/df3d_hip.h, a14): every refusal comes before the device is
touched and names the argument, so these run without a GPU."""
import ctypes

import pytest

P = ctypes.c_void_p
A = 1 << 20   # an address that is never dereferenced: 16-byte aligned, far from the others below


def _buffers(count, step=1 << 24):
    return [A + k * step for k in range(count)]


def _refused(lib, rc, fragment):
    message = lib.df3d_last_error().decode()
    assert rc == -1 and fragment in message, (rc, message)


def test_work_bytes(native_lib):
    lib = native_lib
    slice_ = 2048
    assert lib.df3d_bseg_work_bytes(-1, 16) == 0 and lib.df3d_bseg_work_bytes(10, 1) == 0 and lib.df3d_bseg_work_bytes(10, 1025) == 0
    assert lib.df3d_bseg_work_bytes(65535 * slice_ + 1, 16) == 0
    for G in (2, 33, 256, 1024):
        one = lib.df3d_bseg_work_bytes(slice_, G)
        assert one >= 64 + G * G * 8 and one >= 3 * G * G * 4 and one % 16 == 0
        assert 0 < lib.df3d_bseg_work_bytes(0, G) <= lib.df3d_bseg_work_bytes(1, G) <= one
    # the density's share grows by one [G, G] slice per 2 048 frames: the slice length is a constant of the file
    G = 256
    assert lib.df3d_bseg_work_bytes(3 * slice_ + 1, G) - lib.df3d_bseg_work_bytes(3 * slice_, G) == G * G * 8
    assert lib.df3d_bseg_work_bytes(3 * slice_, G) == lib.df3d_bseg_work_bytes(2 * slice_ + 1, G)
    assert lib.df3d_bseg_work_bytes(100000, G) == 64 + 49 * G * G * 8
    assert lib.df3d_bseg_work_bytes(1 << 20, 2) >= 3 * 4 * (1 << 20) + 4 * (1 << 12)   # the bouts' flags, numbers, starts and block sums


def test_density_and_bounds_refusals(native_lib):
    lib = native_lib
    Y, rho, work, bounds = _buffers(4)
    need = lib.df3d_bseg_work_bytes(100, 16)
    ok = dict(Y=Y, T=100, x0=0.0, y0=0.0, h=0.5, G=16, sigma=1.0, rho=rho, work=work, need=need)

    def call(**kw):
        a = {**ok, **kw}
        return lib.df3d_bseg_density(a["Y"], a["T"], a["x0"], a["y0"], a["h"], a["G"], a["sigma"], a["rho"], a["work"], a["need"], None)

    for G in (1, 0, -5, 1025):
        _refused(lib, call(G=G), "G must be in [2, 1024]")
    for sigma in (0.0, -1.0, float("nan"), float("inf"), 1e-200, 1e200):
        _refused(lib, call(sigma=sigma), "sigma must be finite and > 0")
    for h in (0.0, -0.5, float("nan"), float("inf")):
        _refused(lib, call(h=h), "h must be finite and > 0")
    _refused(lib, call(x0=float("nan")), "x0 and y0 must be finite")
    _refused(lib, call(y0=float("inf")), "x0 and y0 must be finite")
    _refused(lib, call(T=-1), "T must be in")
    _refused(lib, call(T=65535 * 2048 + 1), "T must be in")
    _refused(lib, call(Y=None), "null pointer: Y")
    _refused(lib, call(rho=None), "null pointer: rho")
    _refused(lib, call(work=None), "null pointer: work")
    _refused(lib, call(Y=Y + 8), "Y must be 16-byte aligned")
    _refused(lib, call(rho=rho + 4), "rho must be 8-byte aligned")
    _refused(lib, call(work=work + 8), "work must be 16-byte aligned")
    _refused(lib, call(rho=Y + 16 * 50), "rho must not overlap Y")
    _refused(lib, call(work=rho + 8 * 16), "work must not overlap rho")
    # the query covers every entry; the density itself needs a header of 64 bytes and one [G, G] slice per 2 048 frames
    _refused(lib, call(need=64 + 16 * 16 * 8 - 1), "work buffer too small (df3d_bseg_work_bytes)")
    _refused(lib, call(T=5000, need=64 + 2 * 16 * 16 * 8), "work buffer too small")   # three slices, room for two
    assert call(T=0, Y=None, rho=None, work=None, need=0) == 0   # no frames: nothing is launched
    _refused(lib, lib.df3d_bseg_bounds(None, 5, bounds, None), "null pointer: Y")
    _refused(lib, lib.df3d_bseg_bounds(Y, 5, None, None), "null pointer: bounds")
    _refused(lib, lib.df3d_bseg_bounds(Y, 5, bounds + 4, None), "bounds must be 8-byte aligned")
    _refused(lib, lib.df3d_bseg_bounds(Y, 5, Y + 32, None), "bounds must not overlap Y")
    _refused(lib, lib.df3d_bseg_bounds(Y, -2, bounds, None), "T must be in")
    assert lib.df3d_bseg_bounds(None, 0, None, None) == 0


def test_watershed_refusals(native_lib):
    lib = native_lib
    rho, regions, count, roots, work = _buffers(5)
    need = lib.df3d_bseg_work_bytes(0, 64)
    ok = dict(rho=rho, G=64, min_peak=0.01, regions=regions, count=count, roots=roots, work=work, need=need)

    def call(**kw):
        a = {**ok, **kw}
        return lib.df3d_bseg_watershed(a["rho"], a["G"], a["min_peak"], a["regions"], a["count"], a["roots"], a["work"], a["need"], None)

    for G in (1, 1025, -1):
        _refused(lib, call(G=G), "G must be in [2, 1024]")
    for m in (-0.1, 1.5, float("nan"), float("inf")):
        _refused(lib, call(min_peak=m), "min_peak must be in [0, 1]")
    for name in ("rho", "regions", "roots", "work"):
        _refused(lib, call(**{name: None}), "null pointer: " + {"roots": "root_cells"}.get(name, name))
    _refused(lib, call(count=None), "null pointer: num_regions")
    _refused(lib, call(rho=rho + 4), "rho must be 8-byte aligned")
    _refused(lib, call(regions=regions + 2), "regions must be 4-byte aligned")
    _refused(lib, call(roots=regions + 4 * 64 * 64 - 4), "root_cells must not overlap regions")
    _refused(lib, call(count=regions + 8), "num_regions must not overlap regions")
    _refused(lib, call(need=lib.df3d_bseg_work_bytes(0, 32)), "work buffer too small (df3d_bseg_work_bytes)")


def test_labels_and_bouts_refusals(native_lib):
    lib = native_lib
    Y, regions, labels, bouts, count, occ, tr, work = _buffers(8)
    _refused(lib, lib.df3d_bseg_labels(Y, 10, 0.0, 0.0, 0.5, 1, regions, labels, None), "G must be in [2, 1024]")
    _refused(lib, lib.df3d_bseg_labels(Y, 10, 0.0, 0.0, 0.0, 16, regions, labels, None), "h must be finite and > 0")
    _refused(lib, lib.df3d_bseg_labels(Y, 10, float("nan"), 0.0, 0.5, 16, regions, labels, None), "x0 and y0 must be finite")
    _refused(lib, lib.df3d_bseg_labels(Y, -1, 0.0, 0.0, 0.5, 16, regions, labels, None), "T must be in")
    _refused(lib, lib.df3d_bseg_labels(Y, 1 << 31, 0.0, 0.0, 0.5, 16, regions, labels, None), "T must be in")
    _refused(lib, lib.df3d_bseg_labels(Y, 10, 0.0, 0.0, 0.5, 16, None, labels, None), "null pointer: regions")
    _refused(lib, lib.df3d_bseg_labels(Y, 10, 0.0, 0.0, 0.5, 16, regions, None, None), "null pointer: labels")
    _refused(lib, lib.df3d_bseg_labels(Y + 8, 10, 0.0, 0.0, 0.5, 16, regions, labels, None), "Y must be 16-byte aligned")
    _refused(lib, lib.df3d_bseg_labels(Y, 10, 0.0, 0.0, 0.5, 16, regions, regions + 64, None), "labels must not overlap regions")
    assert lib.df3d_bseg_labels(None, 0, 0.0, 0.0, 0.5, 16, None, None, None) == 0
    need = lib.df3d_bseg_work_bytes(1000, 2)

    def call(labels=labels, T=1000, R=3, bouts=bouts, count=count, occ=occ, tr=tr, work=work, need=need):
        return lib.df3d_bseg_bouts(labels, T, R, bouts, count, occ, tr, work, need, None)

    _refused(lib, call(T=-1), "T must be in")
    _refused(lib, call(R=-1), "num_regions must be in [0, 32 767]")
    _refused(lib, call(R=32768), "num_regions must be in [0, 32 767]")
    for name, shown in (("labels", "labels"), ("bouts", "bouts"), ("count", "num_bouts"), ("occ", "occupancy"), ("tr", "transitions"), ("work", "work")):
        _refused(lib, call(**{name: None}), "null pointer: " + shown)
    _refused(lib, call(bouts=bouts + 4), "bouts must be 8-byte aligned")
    _refused(lib, call(occ=bouts + 8 * 3 * 999), "occupancy must not overlap bouts")
    _refused(lib, call(tr=occ + 8 * 3), "transitions must not overlap occupancy")
    _refused(lib, call(need=need - 1), "work buffer too small (df3d_bseg_work_bytes)")
    assert call(T=0, labels=None, bouts=None, count=None, occ=None, tr=None, work=None, need=0) == 0


def test_the_new_entries_keep_the_abi_revision(native_lib):
    from deepfly3d_amd import _native

    assert native_lib.df3d_version() == _native.ABI_VERSION == 610
    for name in ("df3d_bseg_work_bytes", "df3d_bseg_bounds", "df3d_bseg_density", "df3d_bseg_watershed", "df3d_bseg_labels", "df3d_bseg_bouts"):
        assert name in _native.PROTOTYPES and hasattr(native_lib, name)
    with pytest.raises(ctypes.ArgumentError):
        native_lib.df3d_bseg_work_bytes("many", 16)
