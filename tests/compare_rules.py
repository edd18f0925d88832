"""Comparison rules.  They are different rules, each named for what it holds: ``check_scaled`` is the project's
tolerance of DESIGN.md 5, ``|got - want| <= tol * (max(1, rms(want)) + |want|)`` with the tolerance the caller passes
(``tol_of``: 1e-4 for float32, 1e-2 for 16-bit storage); ``check_f16`` the same form with the tolerance of the tensor's
own type (``tol_of_f16``) and an optional mask; ``close_parity`` the largest error over the largest expectation against
``PARITY_TOL`` of the type; ``check_onepass`` what bench.parity_report reports, each against its own tolerance;
``within`` an allowance per element, with ``report_bound``, ``must_be_zero`` and ``exact_zeros`` beside it."""
import numpy as np
import torch

import bench
import error_bounds as eb
from route_vocab import F16


def tol_of(dtype):
    return 1e-4 if dtype == torch.float32 else 1e-2


def check_scaled(got, want, tol, what):
    got = got.detach().double().cpu().numpy().reshape(np.shape(want))
    want = np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), what
    scale = max(1.0, float(np.sqrt(np.mean(want * want))))
    worst = float((np.abs(got - want) / (scale + np.abs(want))).max())
    print("%s: worst |err| / (%.3g + |want|) = %.3e (tol %.0e)" % (what, scale, worst, tol))
    assert worst <= tol, "%s: worst |err| / (%.3g + |want|) = %.3e > %.1e" % (what, scale, worst, tol)


def rounded(a, dtype):
    """The float64 numbers a tensor of `dtype` holds after taking `a`."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype).double().numpy()


PARITY_TOL = {torch.float64: 1e-10, torch.float32: 1e-4, torch.bfloat16: 1e-2}


def close_parity(got, want, dtype, what, ignore=None):
    """``ignore``: boolean mask (broadcastable to ``want``) of entries excluded from the check."""
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if ignore is not None:
        keep = ~np.broadcast_to(ignore, want.shape)
        got, want = got * keep, want * keep
    scale = max(1.0, float(np.abs(want).max()) if want.size else 1.0)
    err = float(np.abs(got - want).max()) / scale if want.size else 0.0
    assert err <= PARITY_TOL[dtype], "%s: max scaled err %.3e > %.1e" % (what, err, PARITY_TOL[dtype])


POINT_TOL = 1e-4


def report_bound(route, dtype, name, worst):
    print("error-bound | %s | %s | %s | %.3f" % (route, eb.store_name(dtype), name, worst))


def within(got, want, allowance, what):
    """Assert |got - want| <= allowance per element; -> the worst ratio."""
    got = eb.f64(got).reshape(want.shape)
    err = np.abs(got - want)
    assert np.isfinite(got).all(), what
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / allowance)
    worst = float(r.max()) if r.size else 0.0
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    assert worst <= 1.0, "%s: %d of %d elements outside the allowance; worst at %s: got %.9g, want %.9g, allowed %.3e" \
        % (what, int((r > 1).sum()), r.size, at, got[at], want[at], np.broadcast_to(allowance, want.shape)[at])
    return worst


def must_be_zero(ref):
    return int(((ref["A"] + ref["E"]) == 0).sum())


def exact_zeros(g, got, loc64, what):
    """Zeros where the model says zero: the size gradients of a box of decoded size <= 0, all of a row whose window
    lies wholly outside the map, and the angle offset's gradient in mode 1 only."""
    goff, rows, glog = (t.cpu().numpy() for t in got)
    ref, off = g["ref"], g["off"]
    r = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]
    f = np.float32
    w = np.broadcast_to(r[..., 2], off.shape[:4]) + off[..., 2] / f(8) * r[..., 2]
    h = np.broadcast_to(r[..., 3], off.shape[:4]) + off[..., 3] / f(8) * r[..., 3]
    assert (w <= 0).any() and (h <= 0).any(), what
    assert not goff[..., 2][w <= 0].any() and not goff[..., 3][h <= 0].any(), "%s: relu' leaks" % what
    size = np.asarray(g["shapes"], dtype=np.float64)[None, None, None, :, None, ::-1]
    pix = loc64 * size - 0.5
    outside = ((pix <= -1) | (pix >= size)).any(-1).all(-1)             # (B,Lq,H,L): every point of the row outside
    assert outside.any(), what
    assert not goff[outside].any() and not rows[outside].any(), "%s: a row outside the map has a gradient" % what
    assert goff.shape[-1] == (5 if g["angle_mode"] == 1 else 4), (goff.shape, g["angle_mode"])
    assert not rows[..., 4].any() if g["angle_mode"] == 0 else rows[..., 4].any(), what
    if goff.shape[-1] == 5:
        assert goff[..., 4].any(), what


def must_be_zero_share(ref):
    return float(((ref["A"] + ref["E"]) == 0).mean())


def tol_of_f16(t):
    return 1e-3 if t.dtype == F16 else 1e-4


def check_f16(got, want, what, ignore=None):
    tol = tol_of_f16(got)
    got = got.detach().double().cpu().numpy().reshape(np.shape(want))
    want = np.asarray(want, dtype=np.float64)
    if ignore is not None:
        keep = ~np.broadcast_to(ignore, want.shape)
        got, want = got * keep, want * keep
    assert np.isfinite(got).all(), what
    scale = max(1.0, float(np.sqrt(np.mean(want * want)))) if want.size else 1.0
    ratio = np.abs(got - want) / (scale + np.abs(want))
    worst = float(ratio.max()) if want.size else 0.0
    assert worst <= tol, "%s: worst |err| / (%.3g + |want|) = %.3e > %.1e" % (what, scale, worst, tol)


def check_onepass(inp, out, grads, what):
    for name, worst, tol in bench.parity_report(inp, out, grads):
        assert worst <= tol, "%s: %s worst |err| / (max(1, rms) + |want|) = %.3e > %.0e" % (what, name, worst, tol)


def rounded_from_f32(a, dtype):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dtype).double().numpy()
