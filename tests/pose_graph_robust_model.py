"""Referee of the robust loop factors and of the damped solve (include/lili_hip.h: lili_pose_graph_add_loop_robust, lili_pose_graph_loop_status,
lili_pose_graph_solve_lm), on top of tests/pose_graph_model.py.

A loop may carry a loss (GTSAM's noiseModel::Robust).  With r = e / s its whitened residual, d^2 = |r|^2, d = sqrt(d^2), k the scale:
    Huber          w = 1 if d <= k else k / d        rho = d^2 / 2 if d <= k else k (d - k / 2)
    Cauchy         w = k^2 / (k^2 + d^2)             rho = (k^2 / 2) log1p(d^2 / k^2)
    Geman-McClure  w = (k^2 / (k^2 + d^2))^2         rho = (k^2 / 2) d^2 / (k^2 + d^2)
The factor is linearised as sqrt(w) r, sqrt(w) J and adds rho to the cost; every other factor adds |r|^2 / 2."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import pose_graph_model as M

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3
LOSSES = {"none": NONE, "huber": HUBER, "cauchy": CAUCHY, "geman_mcclure": GEMAN_MCCLURE}
LAMBDA_LIMIT = 8


def loss_weight(kind, k, d2):
    d2 = np.asarray(d2, np.float64)
    if kind == NONE:
        return np.ones_like(d2)
    if kind == HUBER:
        d = np.sqrt(d2)
        return np.where(d <= k, 1.0, k / np.where(d > 0, d, 1.0))
    u = k * k / (k * k + d2)
    return u if kind == CAUCHY else u * u


def loss_rho(kind, k, d2):
    d2 = np.asarray(d2, np.float64)
    if kind == NONE:
        return 0.5 * d2
    if kind == HUBER:
        d = np.sqrt(d2)
        return np.where(d <= k, 0.5 * d2, k * (d - 0.5 * k))
    if kind == CAUCHY:
        return 0.5 * k * k * np.log1p(d2 / (k * k))
    return 0.5 * k * k * d2 / (k * k + d2)


class RobustGraph(M.Graph):
    """M.Graph whose loops carry (loss kind, scale); losses[l] belongs to loops[l]"""

    def __init__(self, prior_var=M.PRIOR_VAR, odom_var=M.ODOM_VAR):
        super().__init__(prior_var, odom_var)
        self.losses = []

    def copy(self):
        g = RobustGraph(self.prior_var, self.odom_var)
        g.X, g.meas, g.loops, g.losses = self.X.copy(), self.meas.copy(), list(self.loops), list(self.losses)
        return g

    def add_loop(self, a, b, meas, var, loss=NONE, scale=1.0):
        super().add_loop(a, b, meas, var)
        self.losses.append((int(loss), float(scale)))

    def loop_status(self, X=None):
        """chi2 = d^2 and the weight of every loop at X"""
        X = self.X if X is None else X
        A, B, Z, w, _, _ = self.factors(X)
        r = (M.factor_error(A, B, Z)[0] * w)[self.n:]
        d2 = np.sum(r * r, axis=1)
        wl = np.array([float(loss_weight(kind, k, d2[l])) for l, (kind, k) in enumerate(self.losses)]).reshape(-1)
        return d2, wl

    def cost(self, X):
        A, B, Z, w, _, _ = self.factors(X)
        sq = (M.factor_error(A, B, Z)[0] * w) ** 2
        rho = 0.0
        for l, (kind, k) in enumerate(self.losses):
            if kind != NONE:
                rho += float(loss_rho(kind, k, np.sum(sq[self.n + l])))
                sq[self.n + l] = 0.0
        return 0.5 * float(np.sum(sq)) + rho

    def linearize(self, X):
        r, Ja, Jb, a, b = super().linearize(X)
        for l, (kind, k) in enumerate(self.losses):
            if kind != NONE:
                f = self.n + l
                sw = np.sqrt(float(loss_weight(kind, k, np.sum(r[f] * r[f]))))
                r[f], Ja[f], Jb[f] = r[f] * sw, Ja[f] * sw, Jb[f] * sw
        return r, Ja, Jb, a, b

    def evaluate(self, X=None):
        X = self.X if X is None else X
        _, g, D, S, LB = super().evaluate(X)
        return self.cost(X), g, D, S, LB

    def hessian(self, X=None):
        """the dense weighted H = J^T W J"""
        _, J = self.jacobian(self.X if X is None else X)
        return (J.T @ J).toarray()


def damped_step(H, g, lam, diagonal, solver):
    """delta of (H + damping) delta = -g as M.linear_step solves it; None on a matrix that is not positive definite"""
    d = H.diagonal()
    Hd = (H + sp.diags(lam * d if diagonal else np.full(d.shape, lam))).tocsc()
    if solver == "dense":
        A = Hd.toarray()
        try:
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return None
        return np.linalg.solve(A, -g)
    x = spla.spsolve(Hd, -g, permc_spec="NATURAL" if solver == "natural" else "COLAMD")
    if not np.all(np.isfinite(x)) or float(x @ (Hd @ x)) <= 0:
        return None
    return x


def levenberg_marquardt(graph, X0=None, max_iterations=10, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, initial_lambda=1e-5,
                        lambda_factor=10.0, lambda_lower=1e-10, lambda_upper=1e8, diagonal_damping=0, solver="sparse"):
    """The header's loop (lili_pose_graph_solve_lm).  -> X, summary: M.gauss_newton's entries with one cost / step_inf / grad_inf per ATTEMPT, lambda and accepted per
    attempt, steps_accepted, steps_rejected, final_lambda; `margins` as M.gauss_newton records them, an ("increase", new_cost, cost) entry for every accept / reject
    decision."""
    X = (graph.X if X0 is None else np.asarray(X0, np.float64)).copy()
    cost = graph.cost(X)
    lam = float(initial_lambda)
    s = dict(iterations=0, termination=M.MAX_ITERATIONS, initial_cost=cost, final_cost=cost, cost=[], step_inf=[], grad_inf=[], margins=[], accepted=[],
             steps_accepted=0, steps_rejected=0, final_lambda=lam)
    s["lambda"] = []
    for it in range(max_iterations):
        r, J = graph.jacobian(X)
        H, g = (J.T @ J).tocsc(), J.T @ r
        gmax = float(np.abs(g).max())
        s["grad_inf"].append(gmax)
        s["margins"].append(("gradient", gmax, gradient_tolerance))
        if gmax <= gradient_tolerance:
            s["termination"] = M.GRADIENT_TOLERANCE
            break
        delta = damped_step(H, g, lam, diagonal_damping, solver)
        new_cost, smax, accept = cost, 0.0, False
        if delta is not None:
            Xn = M.retract(X, delta.reshape(-1, 6))
            new_cost, smax = graph.cost(Xn), float(np.abs(delta).max())
            s["margins"].append(("increase", new_cost, cost))
            accept = new_cost <= cost
        s["cost"].append(new_cost); s["step_inf"].append(smax); s["lambda"].append(lam); s["accepted"].append(int(accept))
        s["iterations"] = it + 1
        if accept:
            s["steps_accepted"] += 1
            lam = max(lam / lambda_factor, lambda_lower)
            s["final_lambda"] = lam
            X, old, cost = Xn, cost, new_cost
            s["final_cost"] = cost
            s["margins"].append(("parameter", smax, parameter_tolerance))
            if smax <= parameter_tolerance:
                s["termination"] = M.PARAMETER_TOLERANCE
                break
            s["margins"].append(("function", abs(old - new_cost), function_tolerance * old))
            if abs(old - new_cost) <= function_tolerance * old:
                s["termination"] = M.FUNCTION_TOLERANCE
                break
        else:
            s["steps_rejected"] += 1
            lam = lam * lambda_factor
            s["final_lambda"] = lam
            if lam > lambda_upper:
                s["termination"] = LAMBDA_LIMIT
                break
        if it + 1 >= max_iterations:
            s["termination"] = M.MAX_ITERATIONS
            break
    return X, s
