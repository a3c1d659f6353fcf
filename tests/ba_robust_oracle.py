"""Float64 numpy model of the robust-loss bundle adjustment: scipy's
    least_squares(method='trf', tr_solver='lsmr', x_scale='jac', ftol=1e-4, loss=..., f_scale=...)
restated on the block Jacobian of oracle/trf_lsmr.py.  TEST INFRASTRUCTURE ONLY.

With C = f_scale and z = (f / C)^2 PER SCALAR RESIDUAL (scipy applies rho to each component, not to the 2-D norm):
    cost = 1/2 C^2 sum rho(z)         w = rho'(z)         s^2 = rho' + 2 z rho'', clamped below at EPS = 2^-52
    J's row times s, f <- f w / s
The scaled (J, f) feed g, x_scale='jac', the Cauchy damping, LSMR, the 2-D subspace and the predicted reduction; the actual reduction is
the robust cost of the UNSCALED trial residuals; after an accepted step the unscaled f is re-scaled with the new J.
s^2 is written in closed form per loss (scipy's huber value beyond z = 1 is a difference of equal numbers: rounding noise compared
with EPS); tests/test_ba_robust_host.py pins the closed forms and rho, rho' to scipy's own functions away from the clamp, and the whole
solver to scipy.optimize.least_squares.  deepfly3d_amd/csrc/ba_robust.hip + bundle_adjust.py mirror THIS file step for step."""
import numpy as np

from oracle import geometry as og
from oracle.trf_lsmr import BlockJacobian, eval_blocks, lsmr, solve_trust_region_2d

EPS = np.finfo(np.float64).eps
LOSSES = ("linear", "soft_l1", "huber", "cauchy", "arctan")      # the codes of include/df3d_hip.h: DF3D_BA_LOSS_* = the index here


def rho(loss, z):
    z = np.asarray(z, np.float64)
    if loss == "linear":
        return z.copy()
    if loss == "soft_l1":
        return 2.0 * (np.sqrt(1.0 + z) - 1.0)
    if loss == "huber":
        return np.where(z <= 1.0, z, 2.0 * np.sqrt(z) - 1.0)
    if loss == "cauchy":
        return np.log1p(z)
    if loss == "arctan":
        return np.arctan(z)
    raise ValueError(loss)


def weight(loss, z):
    """rho'(z)"""
    z = np.asarray(z, np.float64)
    if loss == "linear":
        return np.ones_like(z)
    if loss == "soft_l1":
        return 1.0 / np.sqrt(1.0 + z)
    if loss == "huber":
        with np.errstate(divide="ignore"):
            return np.where(z <= 1.0, 1.0, 1.0 / np.sqrt(z))
    if loss == "cauchy":
        return 1.0 / (1.0 + z)
    if loss == "arctan":
        return 1.0 / (1.0 + z * z)
    raise ValueError(loss)


def s2_closed(loss, z):
    """rho' + 2 z rho'' in closed form, NOT clamped."""
    z = np.asarray(z, np.float64)
    if loss == "linear":
        return np.ones_like(z)
    if loss == "soft_l1":
        t = 1.0 + z
        return 1.0 / (t * np.sqrt(t))
    if loss == "huber":
        return np.where(z <= 1.0, 1.0, EPS)
    if loss == "cauchy":
        t = 1.0 + z
        return (1.0 - z) / (t * t)
    if loss == "arctan":
        z2 = z * z
        t = 1.0 + z2
        return (1.0 - 3.0 * z2) / (t * t)
    raise ValueError(loss)


def row_scale(loss, f, f_scale):
    """z, w = rho', s = sqrt(max(s^2, EPS)) and the mask of the clamped rows, per scalar residual."""
    z = (f / f_scale) ** 2
    s2 = s2_closed(loss, z)
    clamped = s2 <= EPS                                  # (huber beyond z = 1 IS the clamp's value)
    s = np.sqrt(np.where(clamped, EPS, s2))
    return z, weight(loss, z), s, clamped


def robust_cost(loss, f, f_scale):
    return 0.5 * f_scale**2 * np.sum(rho(loss, (f / f_scale) ** 2))


def scale_rows(loss, f_scale, f, Jc, Jp):
    """Scaled f (2n,), Jc (n, 2, 6), Jp (n, 2, 3), the weights (2n,) and the clamped mask (2n,)."""
    z, w, s, clamped = row_scale(loss, f, f_scale)
    s2d = s.reshape(-1, 2)
    return f * w / s, Jc * s2d[:, :, None], Jp * s2d[:, :, None], w, clamped


def trf_lsmr_robust(evaluate, x0, loss, f_scale, ftol=1e-4, xtol=1e-8, gtol=1e-8, max_nfev=None):
    """oracle.trf_lsmr.trf_lsmr with scipy's robust-loss scheme.  evaluate(x, want_jac) -> (f, Jc, Jp, make_J) with make_J(Jc, Jp) a
    BlockJacobian.  Returns trf_lsmr's dict plus weights (of the final unscaled residuals) and f (unscaled)."""
    x = x0.copy()
    f_true, Jc, Jp, make_J = evaluate(x, True)
    nfev = njev = 1
    cost = robust_cost(loss, f_true, f_scale)
    f, Jc, Jp, w, _ = scale_rows(loss, f_scale, f_true, Jc, Jp)
    J = make_J(Jc, Jp)
    m, n = J.shape
    gvec = J.rmatvec(f)
    scale_inv = np.sqrt(J.colsq())
    scale_inv[scale_inv == 0] = 1
    scale = 1.0 / scale_inv
    Delta = np.linalg.norm(x0 * scale_inv)
    if Delta == 0:
        Delta = 1.0
    if max_nfev is None:
        max_nfev = x0.size * 100
    status = None
    lsmr_iters = []
    while True:
        g_norm = np.linalg.norm(gvec, ord=np.inf)
        if g_norm < gtol:
            status = 1
        if status is not None or nfev == max_nfev:
            break
        d = scale
        g_h = d * gvec
        mv = lambda v: J.matvec(d * v)  # noqa: E731
        rmv = lambda u: d * J.rmatvec(u)  # noqa: E731
        Jg = mv(-g_h)
        a = 0.5 * (Jg @ Jg)
        b = -(g_h @ g_h)
        to_tr = Delta / np.linalg.norm(g_h)
        cand = [0.0, to_tr]
        if a != 0:
            ext = -0.5 * b / a
            if 0 < ext < to_tr:
                cand.append(ext)
        cand = np.asarray(cand)
        ag_value = np.min(cand * (a * cand + b))
        reg_term = -ag_value / Delta**2
        damp = np.sqrt(reg_term)
        gn_h, istop, itn = lsmr(mv, rmv, f, m, n, damp=damp)[:3]
        lsmr_iters.append(itn)
        S = np.vstack((g_h, gn_h)).T
        S, _ = np.linalg.qr(S, mode="reduced")
        JS = np.stack([mv(S[:, 0]), mv(S[:, 1])], axis=1)
        B_S = JS.T @ JS
        g_S = S.T @ g_h
        actual_reduction = -1.0
        while actual_reduction <= 0 and nfev < max_nfev:
            p_S, _ = solve_trust_region_2d(B_S, g_S, Delta)
            step_h = S @ p_S
            Js = mv(step_h)
            predicted_reduction = -(0.5 * (Js @ Js) + step_h @ g_h)
            step = d * step_h
            x_new = x + step
            f_new = evaluate(x_new, False)[0]
            nfev += 1
            step_h_norm = np.linalg.norm(step_h)
            if not np.all(np.isfinite(f_new)):
                Delta = 0.25 * step_h_norm
                continue
            cost_new = robust_cost(loss, f_new, f_scale)
            actual_reduction = cost - cost_new
            if predicted_reduction > 0:
                ratio = actual_reduction / predicted_reduction
            elif predicted_reduction == actual_reduction == 0:
                ratio = 1
            else:
                ratio = 0
            Delta_new = Delta
            if ratio < 0.25:
                Delta_new = 0.25 * step_h_norm
            elif ratio > 0.75 and step_h_norm > 0.95 * Delta:
                Delta_new = 2.0 * Delta
            step_norm = np.linalg.norm(step)
            ftol_ok = actual_reduction < ftol * cost and ratio > 0.25
            xtol_ok = step_norm < xtol * (xtol + np.linalg.norm(x))
            if ftol_ok and xtol_ok:
                status = 4
            elif ftol_ok:
                status = 2
            elif xtol_ok:
                status = 3
            if status is not None:
                break
            Delta = Delta_new
        if actual_reduction > 0:
            x = x_new
            cost = cost_new
            f_true, Jc, Jp, make_J = evaluate(x, True)
            njev += 1
            f, Jc, Jp, w, _ = scale_rows(loss, f_scale, f_true, Jc, Jp)
            J = make_J(Jc, Jp)
            gvec = J.rmatvec(f)
            scale_inv = np.maximum(np.sqrt(J.colsq()), scale_inv)
            scale = 1.0 / scale_inv
    if status is None:
        status = 0
    return dict(x=x, cost=cost, nfev=nfev, njev=njev, status=status, lsmr_iters=lsmr_iters, optimality=g_norm, weights=w, f=f_true)


def problem(points2d_px, R, tvec, intr, pts0=None):
    """The adjustment's tables and start vector, as oracle.trf_lsmr.bundle_adjust sets them up (pts0: start points, default the DLT's)."""
    R, tvec, intr = np.asarray(R, np.float64), np.asarray(tvec, np.float64), np.asarray(intr, np.float64)
    ncam = R.shape[0]
    if pts0 is None:
        pts0 = og.triangulate_dlt_batched(points2d_px, og.projection_matrices(R, tvec, intr))
    cam_idx, pt_idx, obs_xy, slot = og.build_observations(points2d_px)
    x0 = og.ba_pack(R, tvec, pts0, slot)
    npts = int((slot >= 0).sum())

    def evaluate(x, want_jac):
        if not want_jac:
            return og.ba_residuals(x, ncam, intr, cam_idx, pt_idx, obs_xy), None, None, None
        r, Jc, Jp = eval_blocks(x, ncam, intr, cam_idx, pt_idx, obs_xy)
        return r, Jc, Jp, lambda a, b: BlockJacobian(ncam, npts, cam_idx, pt_idx, a, b)

    return dict(ncam=ncam, npts=npts, cam_idx=cam_idx, pt_idx=pt_idx, obs_xy=obs_xy, slot=slot, x0=x0, intr=intr, evaluate=evaluate)


def bundle_adjust(points2d_px, R, tvec, intr, loss="soft_l1", f_scale=1.0, pts0=None):
    """R, tvec, info of the robust adjustment (info as trf_lsmr_robust, plus obs_weight: per observation, the smaller of its two
    components' weights)."""
    pr = problem(points2d_px, R, tvec, intr, pts0)
    res = trf_lsmr_robust(pr["evaluate"], pr["x0"], loss, f_scale)
    cams = res["x"][: pr["ncam"] * 6].reshape(pr["ncam"], 6)
    res["obs_weight"] = res["weights"].reshape(-1, 2).min(axis=1)
    res["points"] = res["x"][pr["ncam"] * 6 :].reshape(-1, 3)
    return og.matrix_from_rotvec(cams[:, :3]), cams[:, 3:].copy(), res


def clean_reprojection_error(clean_px, R, tvec, intr):
    """Mean reprojection error of the CLEAN detections, re-triangulated with the given cameras (the figure of the issue's table)."""
    pts = og.triangulate_dlt_batched(clean_px, og.projection_matrices(np.asarray(R), np.asarray(tvec), np.asarray(intr)))
    return og.reprojection_error(clean_px, pts, R, tvec, intr)
