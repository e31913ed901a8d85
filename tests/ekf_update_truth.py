"""An extended-precision truth for the dense EKF update, independent of the kernels under test (plain NumPy, no GPU).

From the PRIOR total state x and covariance P and the records of the features measured in this frame (dh_by_dxp [2][7],
dh_by_dy [2][3], pos, R, nu) it forms, in np.longdouble,

    A = H P,   S = A H^T + R,   S = L L^T,   V = L^-1 A,   w = L^-1 nu,
    P+ = P - V^T V,                      x+ = x + V^T w

which is the chain k_build_AS -> k_chol_left -> k_fwdsub_* -> k_syrk written down once more with sixty-four-bit mantissas and
plain loops.  posterior_truth(e, b) reads an Engine between make_measurements and kalman_filter_update, posterior_truth_of_oracle
(o) an OracleSLAM at the same point, so the truth itself can be exercised without a device.

The bound a posterior is held to is the forward-error shape of a Cholesky solve, the one tests/test_gpu_step_stats.py
uses for the factorisation:

    |P+ - P+_truth|_F   <= c m 2^-53 cond(S) |P_prior|_F
    max |x+ - x+_truth| <= c m 2^-53 cond(S) max(1, |x|_inf)

with cond(S) by np.linalg.cond.  tests/ekf_update_cases.py holds c and says where it comes from."""
import numpy as np

EPS = 2.0 ** -53


def chol_solve_longdouble(S, nu):
    """L (S = L L^T, column by column) and w = L^-1 nu in np.longdouble."""
    m = S.shape[0]
    L = np.zeros((m, m), dtype=np.longdouble)
    for j in range(m):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0
        L[j, j] = np.sqrt(d)
        if j + 1 < m:
            L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    w = np.zeros(m, dtype=np.longdouble)
    for j in range(m):
        w[j] = (nu[j] - L[j, :j] @ w[:j]) / L[j, j]
    return L, w


def forward_substitute_longdouble(L, A):
    """V = L^-1 A, row by row, in np.longdouble (A is [m][n])."""
    V = np.zeros(A.shape, dtype=np.longdouble)
    for j in range(L.shape[0]):
        V[j] = (A[j] - L[j, :j] @ V[:j]) / L[j, j]
    return V


def measured_features(e, b):
    """The features of sequence b of an Engine that this frame's update uses: feature_list_ order = slot order = the rows' order."""
    return [f for f in e.features(b) if f["selected"] and f["success"]]


def measured_features_of_oracle(o):
    """The same records from an OracleSLAM (its Jacobian with respect to the vehicle state is [2][13]: the pose's seven columns
    are the non-zero ones)."""
    out = []
    for i in range(o.num_features):
        f = o.feature(i)
        if f["selected"] and f["success"]:
            assert not f["dh_by_dxv"][:, 7:].any()
            f["dh_by_dxp"] = f["dh_by_dxv"][:, :7]
            out.append(f)
    return out


def innovation_system(P, ok):
    """A = H P [m][n], S = H P H^T + R [m][m] and nu [m] in np.longdouble, from the prior covariance P (any float type) and the
    records `ok` of the measured features (ten non-zeros per row of H: seven pose columns and the feature's three)."""
    P = P.astype(np.longdouble)
    n = P.shape[0]
    Hx = np.concatenate([f["dh_by_dxp"] for f in ok]).astype(np.longdouble)            # [m][7]
    Hy = np.concatenate([f["dh_by_dy"] for f in ok]).astype(np.longdouble)             # [m][3]
    pos = np.repeat([f["pos"] for f in ok], 2)
    assert (pos >= 13).all() and (pos + 3 <= n).all()
    cols = pos[:, None] + np.arange(3)[None, :]                                        # [m][3]
    A = Hx @ P[:7, :] + np.einsum("rk,rkn->rn", Hy, P[cols])                            # H P, row by row
    S = A[:, :7] @ Hx.T + np.einsum("rck,ck->rc", A[:, cols], Hy)                      # (H P) H^T
    S = S + np.diag(np.repeat([f["R"] for f in ok], 2).astype(np.longdouble))
    nu = np.concatenate([f["nu"] for f in ok]).astype(np.longdouble)
    return A, S, nu


def posterior_from(x, P, ok):
    """dict(P, x: the posterior in np.longdouble; m; cond: cond(S); norm_P: |P_prior|_F; x_inf: |x_prior|_inf)."""
    t = dict(m=2 * len(ok), cond=1.0, norm_P=float(np.linalg.norm(P)), x_inf=float(np.abs(x).max()) if x.size else 0.0,
             P=P.astype(np.longdouble), x=x.astype(np.longdouble))
    if not ok:
        return t
    A, S, nu = innovation_system(P, ok)
    L, w = chol_solve_longdouble(S, nu)
    V = forward_substitute_longdouble(L, A)
    t.update(P=t["P"] - V.T @ V, x=t["x"] + V.T @ w, cond=float(np.linalg.cond(S.astype(np.float64))))
    return t


def posterior_truth(e, b):
    """Call between make_measurements and kalman_filter_update: what x and P of sequence b must be after the update."""
    return posterior_from(e.total_state(b), e.total_covariance(b), measured_features(e, b))


def posterior_truth_of_oracle(o):
    """The same from an OracleSLAM's pre-update state."""
    return posterior_from(o.total_state(), o.total_covariance(), measured_features_of_oracle(o))


def bounds(t, c):
    """(bound on |P+ - truth|_F, bound on max |x+ - truth|) for the truth t at the constant c."""
    scale = c * max(t["m"], 1) * EPS * t["cond"]
    return scale * t["norm_P"], scale * max(1.0, t["x_inf"])


def deviation_over_bound(x, P, t, c):
    """(|P - P+_truth|_F / bound, max |x - x+_truth| / bound) of a posterior (x, P) in float64."""
    bP, bx = bounds(t, c)
    dP = float(np.linalg.norm((P.astype(np.longdouble) - t["P"]).astype(np.float64)))
    dx = float(np.abs(x.astype(np.longdouble) - t["x"]).max()) if x.size else 0.0
    return dP / bP if bP > 0 else (0.0 if dP == 0 else np.inf), dx / bx
