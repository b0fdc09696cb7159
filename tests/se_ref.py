"""Extended-precision reference of fields::predictSE.Krig for the TPS standard-error tests (test infrastructure only:
the product never imports it).

On the fit's notation (oracle/tps.py): knots u, weights W = diag(weightsM), K_ij = phi(|u_i - u_j|^2), T = [1 u v],
M = [[K + lambda W^-1, T], [T', 0]] and z(x) = [phi(|(u, v) - u_j|^2)_j ; 1 ; u ; v].  Two forms of the variance:

  literal    var(x) = rho phi(0) - 2 rho k(x)'a(x) + a(x)' (rho K + sigma^2 W^-1) a(x),   a(x) = M^-1[:n, :] z(x)
             (f^(x) = a(x)' yM; predictSE.Krig with the covariance rho phi),
  quadratic  var(x) = -rho z(x)' M^-1 z(x),

equal for rho = sigma^2 / lambda.  M^-1 is computed in long double (Gauss-Jordan with partial pivoting), phi with the
knot convention phi(0) = 0 of oracle.tps._phi_ld.  Scaled point coordinates are formed in float64, as the device
forms them, then carried in long double."""
import numpy as np

from oracle import tps as otps

LD = np.longdouble


def problem(xy, y):
    """The stations as fields' Krig sees them: knots (float64, as the fit's), weightsM, yM, N, pure_ss, transform."""
    xm, ym, w, pure_ss = otps.collapse_replicates(xy, y)
    center, scale = otps.range_scale(xm)
    u = (xm - center) / scale
    return {"knots": u, "w": w, "yM": ym, "N": int(np.asarray(y).size), "pure_ss": pure_ss, "center": center,
            "scale": scale}


def inv_ld(A):
    """Inverse of a square matrix in long double (Gauss-Jordan, partial pivoting)."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    X = np.concatenate([A, np.eye(n, dtype=LD)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(X[k:, k])))
        if p != k:
            X[[k, p]] = X[[p, k]]
        X[k] /= X[k, k]
        col = X[:, k].copy()
        col[k] = 0
        X -= np.outer(col, X[k])
    return X[:, n:]


def saddle_ld(knots, w, lam):
    u = np.asarray(knots, dtype=LD)
    n = u.shape[0]
    dx = u[:, None, 0] - u[None, :, 0]
    dy = u[:, None, 1] - u[None, :, 1]
    M = np.zeros((n + 3, n + 3), dtype=LD)
    M[:n, :n] = otps._phi_ld(dx * dx + dy * dy) + np.diag(LD(lam) / np.asarray(w, dtype=LD))
    T = np.column_stack([np.ones(n, dtype=LD), u])
    M[:n, n:] = T
    M[n:, :n] = T.T
    return M


def z_ld(knots, center, scale, xy):
    """z(x) for every point (rows), u in float64 as the device forms it."""
    uv = (np.asarray(xy, dtype=np.float64).reshape(-1, 2) - center) / scale
    p = uv.astype(LD)
    k = np.asarray(knots, dtype=LD)
    dx = p[:, None, 0] - k[None, :, 0]
    dy = p[:, None, 1] - k[None, :, 1]
    return np.concatenate([otps._phi_ld(dx * dx + dy * dy), np.ones((p.shape[0], 1), dtype=LD), p], axis=1)


class SeReference:
    """M^-1 of one spline (knots, weights, lambda), and the SE quantities at points."""

    def __init__(self, knots, w, lam, center, scale):
        self.knots, self.w, self.lam = np.asarray(knots), np.asarray(w, dtype=np.float64), float(lam)
        self.center, self.scale = np.asarray(center), np.asarray(scale)
        self.n = self.knots.shape[0]
        self.M = saddle_ld(self.knots, self.w, self.lam)
        self.Minv = inv_ld(self.M)

    def z(self, xy):
        return z_ld(self.knots, self.center, self.scale, xy)

    def var_quadratic(self, xy, sigma2):
        Z = self.z(xy)
        rho = LD(sigma2) / LD(self.lam)
        return -rho * np.einsum("ij,ij->i", Z @ self.Minv, Z)

    def var_literal(self, xy, sigma2):
        Z = self.z(xy)
        n = self.n
        rho = LD(sigma2) / LD(self.lam)
        a = Z @ self.Minv[:, :n]                 # rows a(x)' (M^-1 symmetric)
        k = Z[:, :n]
        K = self.M[:n, :n] - np.diag(LD(self.lam) / self.w.astype(LD))
        Sigma = rho * K + np.diag(LD(sigma2) / self.w.astype(LD))
        return -2 * rho * np.einsum("ij,ij->i", k, a) + np.einsum("ij,ij->i", a @ Sigma, a)   # + rho phi(0) = 0

    def bound(self, xy, sigma2):
        """rho |z|' |M^-1| |z|: the scale of the rounding a float64 evaluation of z' M^-1 z can make."""
        Z = np.abs(self.z(xy))
        return LD(sigma2) / LD(self.lam) * np.einsum("ij,ij->i", Z @ np.abs(self.Minv), Z)

    def sigma2(self, yM, N, pure_ss):
        """(RSS_w + pure_ss) / (N - eff_df) at this lambda: RSS_w = sum w (yM - f^(xM))^2, eff_df = tr A(lambda)."""
        n = self.n
        yl = np.asarray(yM, dtype=LD)
        c = self.Minv[:n, :n] @ yl
        d = self.Minv[n:, :n] @ yl
        K = self.M[:n, :n] - np.diag(LD(self.lam) / self.w.astype(LD))
        T = self.M[:n, n:]
        fhat = K @ c + T @ d
        rss = np.sum(self.w.astype(LD) * (yl - fhat) ** 2)
        eff_df = n - LD(self.lam) * np.sum(np.diag(self.Minv)[:n] / self.w.astype(LD))
        return (rss + LD(pure_ss)) / (LD(N) - eff_df)


def for_fit(xy, y, lam):
    """SeReference of the spline fitted to the stations (xy, y) at lambda, with the problem's yM / N / pure_ss."""
    p = problem(xy, y)
    ref = SeReference(p["knots"], p["w"], lam, p["center"], p["scale"])
    ref.problem = p
    return ref
