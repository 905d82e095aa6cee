"""The trust-region step policy as a numpy model, and scripted records that force each of its branches.

A plain helper module (not a conftest): test_lm_cases.py checks the model and the scenarios on the CPU, test_gpu_lm_steps.py
plays the same scenarios through ll_map_lm_begin / ll_map_lm_propose / ll_map_lm_accept and compares the pose after every call.

The model restates Ceres 2.x trust_region_minimizer.cc with levenberg_marquardt_strategy.cc from their description, not from the
library's or the oracle's code, and factorises nothing by hand: where a record came from a Jacobian (H = J^T J, g = J^T r) the step
is the least-squares solution of the stacked system [J S; sqrt(D)] y = [-r; 0] (numpy.linalg.lstsq, as DENSE_QR takes it), and for
a record with no Jacobian behind it numpy.linalg.solve, with numpy.linalg.eigvalsh deciding whether the factorisation succeeds.

  begin     scale S_i = 1 / (1 + sqrt(H_ii)) once (1 when jacobi_scaling is off), radius = initial_radius, decrease factor 2
  propose   stop when iterations >= max_num_iterations, radius < min_radius or max|Plus(x, -g) - x| <= gradient_tolerance;
            A = S H S, b = S g, A_ii += clamp(A_ii, min_lm_diagonal, max_lm_diagonal) / radius, (A + D) y = -b, d = S y,
            model_cost_change = -(g.d + d.H.d / 2); a failed solve or a change that is not > 0 is an invalid step: the radius is
            halved, x stays and the iteration counts; otherwise the candidate is Plus(x, d)
  accept    on the candidate's record, in this order: |cand - x| <= parameter_tolerance (|x| + parameter_tolerance) stops,
            |cost - cc| <= function_tolerance cost stops (x kept in both), rho = (cost - cc) / model_cost_change > min_relative_decrease
            takes the candidate and its record with radius = min(radius / max(1/3, 1 - (2 rho - 1)^3), max_radius) and the
            factor back at 2, anything else divides the radius by the factor and doubles the factor
A stopped solve ignores every later call and keeps returning x.

A pose is (qx, qy, qz, qw, tx, ty, tz); a step is (three rotation components w, three translation components);
Plus(x, d): q+ = [sin|w| w/|w|, cos|w|] (x) q (the identity when |w| = 0), t += the translation components.
A record is the 44 doubles the stepwise calls take: H 6 x 6 row-major, g, cost, rows.
"""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
INF = float("inf")

# the Ceres defaults as the solves here configure them
DEFAULTS = dict(max_num_iterations=4, initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3,
                min_lm_diagonal=1e-6, max_lm_diagonal=1e32, function_tolerance=1e-6, gradient_tolerance=1e-10,
                parameter_tolerance=1e-8, jacobi_scaling=1)


def options(**kw):
    """the defaults with the given fields replaced"""
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def fill(struct, opt):
    """opt (a dict of options()) into a ctypes options structure (api.LmOptions, orc.LmOptions): every field, none left to a default"""
    for k, v in opt.items():
        setattr(struct, k, v)
    return struct


def qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def plus(x, d):
    x = np.asarray(x, np.float64); d = np.asarray(d, np.float64)
    out = x.copy()
    n = math.sqrt(float(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    if n != 0.0:
        s = math.sin(n) / n
        out[:4] = qmul(np.array([s * d[0], s * d[1], s * d[2], math.cos(n)]), x[:4])
    out[4:] = x[4:] + d[3:]
    return out


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).tolist() == np.ascontiguousarray(b, np.float64).view(np.uint64).tolist()


class Record:
    """normal equations at a pose; J, r: the Jacobian and residuals they came from, where there are any"""

    def __init__(self, H, g, cost, rows=0.0, J=None, r=None):
        self.H = np.array(H, np.float64).reshape(6, 6); self.g = np.array(g, np.float64).reshape(6)
        self.cost = float(cost); self.rows = float(rows)
        self.J = None if J is None else np.array(J, np.float64); self.r = None if r is None else np.array(r, np.float64)

    @classmethod
    def from_jacobian(cls, J, r, cost=None):
        J = np.asarray(J, np.float64); r = np.asarray(r, np.float64)
        H = J.T @ J
        return cls(0.5 * (H + H.T), J.T @ r, 0.5 * float(r @ r) if cost is None else cost, len(r), J, r)

    @classmethod
    def from_vec(cls, v):
        v = np.asarray(v, np.float64)
        return cls(v[:36], v[36:42], v[42], v[43])

    def with_cost(self, cost):
        return Record(self.H, self.g, cost, self.rows, self.J, self.r)

    def vec(self):
        return np.concatenate([self.H.ravel(), self.g, [self.cost, self.rows]])


# wrong policies, each one plausible slip, and the scenarios that must tell it from the right one
MUTANTS = {
    "rescale_on_accept": ["scale_kept"],                  # the Jacobi scale follows the accepted record
    "factor_not_reset": ["reject_chain"],                 # an accepted step leaves the decrease factor where the rejects put it
    "factor_not_doubled": ["reject_chain"],
    "invalid_not_counted": ["invalid_counts_max_2"],      # an invalid step is not an iteration
    "radius_not_capped": ["radius_capped"],
    "radius_not_floored": ["radius_rho_1.5"],             # no max(1/3, .): rho 1.5 would shrink the radius through a negative divisor
    "clamp_before_scaling": ["clamp_max_0.9_jacobi_1"],   # the clamps applied to H_ii, not to the scaled A_ii
    "function_test_first": ["stop_parameter"],            # same stop, another branch: only the log can tell
    "tolerance_after_step": ["stop_function", "plus_far_start_parameter_stop"],   # the tolerance stops take the candidate first
    "infinite_cost_stops": ["infinite_cost"],
}


class LmModel:
    """begin / propose / accept return the pose expected after the call; log: the branch every call took; trace: one dict per
    propose that computed a step (radius, kappa of the damped scaled matrix, the step d, clamped: which clamps were active);
    margins: (what, lhs, rhs) of every tolerance and rho comparison made, for the tests that want a decision far from its threshold"""

    def __init__(self, opt, mutant=None):
        self.o = dict(opt)
        assert mutant is None or mutant in MUTANTS, mutant
        self.mutant = mutant                              # a deliberately wrong policy (MUTANTS), for the tests that show a scenario tells it from the right one
        self.log = []; self.trace = []; self.margins = []; self.costs = []
        self.x = None

    def _scale(self, H):
        return 1.0 / (1.0 + np.sqrt(np.diag(H))) if self.o["jacobi_scaling"] else np.ones(6)

    def begin(self, pose, rec):
        self.x = np.array(pose, np.float64)
        self.rec = rec
        self.S = self._scale(rec.H)
        self.radius = float(self.o["initial_radius"]); self.factor = 2.0
        self.iterations = 0; self.successes = 0; self.done = False; self.pending = False
        self.costs.append(rec.cost)
        self.log.append("begin")
        return self.x.copy()

    def _solve(self):
        """-> (ok, d, kappa, clamped) for the current record, scale and radius"""
        o, S, H, g = self.o, self.S, self.rec.H, self.rec.g
        A = S[:, None] * H * S[None, :]
        dg = np.diag(H).copy() if self.mutant == "clamp_before_scaling" else np.diag(A)
        D = np.minimum(np.maximum(dg, o["min_lm_diagonal"]), o["max_lm_diagonal"]) / self.radius
        clamped = ("min" if (dg < o["min_lm_diagonal"]).any() else "") + ("max" if (dg > o["max_lm_diagonal"]).any() else "")
        # the factorisation of a symmetric matrix reads one triangle, the lower one here as with LAPACK's default; an inconsistent
        # (asymmetric) record shows in model_cost_change, which sums all 36 entries of H
        M = A + np.diag(D)
        M = np.tril(M) + np.tril(M, -1).T
        with np.errstate(all="ignore"):
            finite = bool(np.isfinite(M).all())
            kappa = float(np.linalg.cond(M, 2)) if finite else INF
        if self.rec.J is not None:
            stacked = np.vstack([self.rec.J * S[None, :], np.diag(np.sqrt(D))])
            y = np.linalg.lstsq(stacked, np.concatenate([-self.rec.r, np.zeros(6)]), rcond=None)[0]
            ok = True
        else:
            ok = finite and float(np.linalg.eigvalsh(M).min()) > 0.0
            y = np.linalg.solve(M, -(S * g)) if ok else np.zeros(6)
        return ok, S * y, kappa, clamped

    def propose(self):
        o = self.o
        self.pending = False
        if not self.done:
            grad = float(np.abs(plus(self.x, -self.rec.g) - self.x).max())
            if self.iterations >= o["max_num_iterations"]:
                self.done = True; self.log.append("stop:max_iterations")
            elif self.radius < o["min_radius"]:
                self.done = True; self.log.append("stop:min_radius")
            else:
                self.margins.append(("gradient", grad, o["gradient_tolerance"]))
                if grad <= o["gradient_tolerance"]:
                    self.done = True; self.log.append("stop:gradient")
            if self.done:
                return self.x.copy()
        else:
            self.log.append("done")
            return self.x.copy()
        self.iterations += 1
        ok, d, kappa, clamped = self._solve()
        mcc = -(float(self.rec.g @ d) + 0.5 * float(d @ self.rec.H @ d)) if ok else 0.0
        self.trace.append(dict(radius=self.radius, kappa=kappa, d=d.copy(), clamped=clamped, mcc=mcc, ok=ok, scale=self.S.copy()))
        if not ok or not mcc > 0.0:
            self.radius *= 0.5
            if self.mutant == "invalid_not_counted":
                self.iterations -= 1
            self.log.append("invalid:solve" if not ok else "invalid:model")
            return self.x.copy()
        self.cand = plus(self.x, d); self.mcc = mcc; self.pending = True
        self.log.append("candidate")
        return self.cand.copy()

    def _stopped(self):
        if self.mutant == "tolerance_after_step":
            self.x = self.cand.copy()
        return self.x.copy()

    def accept(self, rec):
        o = self.o
        if self.done or not self.pending:
            self.pending = False
            self.log.append("done" if self.done else "idle")
            return self.x.copy()
        self.pending = False
        cost, cc = self.rec.cost, rec.cost
        if self.mutant == "infinite_cost_stops" and not math.isfinite(cc):
            self.done = True; self.log.append("stop:infinite")
            return self.x.copy()
        if self.mutant == "function_test_first" and abs(cost - cc) <= o["function_tolerance"] * cost:
            self.done = True; self.log.append("stop:function")
            return self.x.copy()
        step_norm = float(np.linalg.norm(self.cand - self.x)); x_norm = float(np.linalg.norm(self.x))
        self.margins.append(("parameter", step_norm, o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"])))
        if step_norm <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            self.done = True; self.log.append("stop:parameter")
            return self._stopped()
        self.margins.append(("function", abs(cost - cc), o["function_tolerance"] * cost))
        if abs(cost - cc) <= o["function_tolerance"] * cost:
            self.done = True; self.log.append("stop:function")
            return self._stopped()
        rho = (cost - cc) / self.mcc
        self.margins.append(("rho", rho, o["min_relative_decrease"]))
        if rho > o["min_relative_decrease"]:
            self.x = self.cand.copy(); self.rec = rec
            f = 1.0 - (2.0 * rho - 1.0) ** 3
            self.radius = self.radius / (f if self.mutant == "radius_not_floored" else max(1.0 / 3.0, f))
            if self.mutant != "radius_not_capped":
                self.radius = min(self.radius, o["max_radius"])
            if self.mutant != "factor_not_reset":
                self.factor = 2.0
            self.successes += 1
            if self.mutant == "rescale_on_accept":
                self.S = self._scale(rec.H)
            self.costs.append(cc)
            self.log.append("accept")
        else:
            self.radius /= self.factor
            if self.mutant != "factor_not_doubled":
                self.factor *= 2.0
            self.log.append("reject")
        return self.x.copy()


def solve(evaluate, pose0, opt):
    """the model as a solver: evaluate(pose) -> Record.  -> (pose, model)"""
    m = LmModel(opt)
    m.begin(pose0, evaluate(np.asarray(pose0, np.float64)))
    while not m.done:
        cand = m.propose()
        if m.pending:
            m.accept(evaluate(cand))
    return m.x.copy(), m


def replay(opt, pose0, records):
    """records: what a stepwise solve evaluated, the begin record first, then one per iteration (at whatever pose the propose left).
    -> the model after begin and len(records) - 1 rounds of (propose, accept)"""
    m = LmModel(opt)
    m.begin(pose0, Record.from_vec(records[0]))
    for v in records[1:]:
        m.propose()
        m.accept(Record.from_vec(v))
    return m


# ----------------------------------------------------------------------------- scripted scenarios
class Step:
    """one round: a propose, then (unless rec is None) an accept with rec, whose cost is cost - rho * model_cost_change of the
    model's own step when rho is given, cost(model) when cost is a callable, or rec's own"""

    def __init__(self, rec=None, rho=None, cost=None):
        self.rec, self.rho, self.cost = rec, rho, cost

    def record(self, m):
        if self.rec is None:
            return None
        if self.rho is not None and m.pending:
            return self.rec.with_cost(m.rec.cost - self.rho * m.mcc)
        if callable(self.cost):
            return self.rec.with_cost(self.cost(m))
        return self.rec


class Scenario:
    def __init__(self, name, opt, pose0, rec0, steps, branches, radii=None):
        self.name, self.opt, self.pose0, self.rec0, self.steps = name, opt, np.array(pose0, np.float64), rec0, steps
        self.branches = branches          # the model's log must be exactly this
        self.radii = radii                # and, where given, the radius of every step computed exactly these


class Stage:
    """one call: which, the branch the model took, the model's pose after it, the device's (None without a device), the
    step's trace entry for a propose that computed one"""

    def __init__(self, call, branch, ref, got, tr):
        self.call, self.branch, self.ref, self.got, self.tr = call, branch, ref, got, tr


def play(sc, dev=None, dev_opt=None, model=None):
    """sc on the model and, with dev (an api.Map), on the device: -> (model, [Stage]).  After an accepted step the model goes on
    from the device's pose, so that every candidate is compared over one step and not over the rounding of the steps before."""
    m = model if model is not None else LmModel(sc.opt)
    stages = []

    def got():
        return None if dev is None else dev.pose()

    ref = m.begin(sc.pose0, sc.rec0)
    if dev is not None:
        dev.set_pose(sc.pose0)
        dev.lm_begin(sc.rec0.vec(), dev_opt)
    stages.append(Stage("begin", m.log[-1], ref, got(), None))
    for st in sc.steps:
        n_tr = len(m.trace)
        ref = m.propose()
        if dev is not None:
            dev.lm_propose(dev_opt)
        stages.append(Stage("propose", m.log[-1], ref, got(), m.trace[-1] if len(m.trace) > n_tr else None))
        rec = st.record(m)
        if rec is None:
            continue
        ref = m.accept(rec)
        if dev is not None:
            dev.lm_accept(rec.vec(), dev_opt)
        stages.append(Stage("accept", m.log[-1], ref, got(), None))
        if dev is not None and m.log[-1] == "accept":
            m.x = stages[-1].got.copy()
    return m, stages


def candidate_bound(tr, pose):
    """64 eps kappa |d|_inf + 8 eps |pose|_inf: the backward-error bound of a 6 x 6 Cholesky solve (relative error of the
    solution <= c n eps kappa, Higham, Accuracy and Stability of Numerical Algorithms, theorem 10.4, with a generous constant)
    plus the rounding of the composition with the pose"""
    return 64.0 * EPS * tr["kappa"] * float(np.abs(tr["d"]).max()) + 8.0 * EPS * float(np.abs(pose).max())


def _pose(rng, t_scale=1.0):
    q = np.concatenate([0.2 * rng.standard_normal(3), [1.0]])
    return np.concatenate([q / np.linalg.norm(q), t_scale * rng.standard_normal(3)])


def _jrec(rng, jscale=1.0, rscale=1.0, cost=None):
    return Record.from_jacobian(jscale * rng.standard_normal((40, 6)), rscale * rng.standard_normal(40), cost)


def _hrec(rng, jscale=1.0, rscale=1.0, g=None, cost=None):
    """a record with no Jacobian behind it (the model takes it with solve / eigvalsh)"""
    r = _jrec(rng, jscale, rscale)
    return Record(r.H, r.g if g is None else g, r.cost if cost is None else cost, r.rows)


def _arbitrary(rng):
    """records a stopped solve must ignore: an attractive one (far lower cost), one that asks for a huge step"""
    return [Step(_jrec(rng, cost=1e-3)), Step(_hrec(rng, jscale=1e-3, rscale=1e3, cost=0.0)), Step(None)]


H_INDEFINITE = np.eye(6); H_INDEFINITE[0, 1] = H_INDEFINITE[1, 0] = 2.5


def scenarios():
    """-> {name: Scenario}, built afresh (and identically) on every call"""
    out = {}

    def add(name, opt, pose0, rec0, steps, branches, radii=None):
        assert name not in out
        out[name] = Scenario(name, opt, pose0, rec0, steps, branches, radii)

    r1 = options(initial_radius=1.0, max_num_iterations=8)

    # 1. the rejects, the doubling factor, the accept, the factor's reset
    rng = np.random.default_rng(101)
    grown = 0.125 / (1.0 - 0.8 ** 3)
    add("reject_chain", r1, _pose(rng), _jrec(rng),
        [Step(_jrec(rng), rho=-1.0), Step(_jrec(rng), rho=5e-4), Step(_jrec(rng), rho=0.9), Step(_jrec(rng), rho=-2.0), Step(_jrec(rng), rho=0.5)],
        ["begin"] + ["candidate", "reject"] * 2 + ["candidate", "accept", "candidate", "reject", "candidate", "accept"],
        [1.0, 0.5, 0.125, grown, grown / 2.0])

    # 2. the radius update: the step after the accepted one shows the new radius
    for name, rho, cap, r_next in (("radius_rho_0.5", 0.5, 1e16, 1.0), ("radius_rho_1.0", 1.0, 1e16, 3.0), ("radius_rho_1.5", 1.5, 1e16, 3.0),
                                   ("radius_rho_2e-3", 2e-3, 1e16, 1.0 / (1.0 - (2.0 * 2e-3 - 1.0) ** 3)), ("radius_capped", 1.0, 2.0, 2.0)):
        rng = np.random.default_rng(102)
        add(name, options(initial_radius=1.0, max_radius=cap), _pose(rng), _jrec(rng), [Step(_jrec(rng), rho=rho), Step(_jrec(rng), rho=0.5)],
            ["begin", "candidate", "accept", "candidate", "accept"], [1.0, r_next])

    # 3. invalid by factorisation: the damped matrix is indefinite at radius 1 and positive definite at 0.5, scaled or not
    for js in (1, 0):
        rng = np.random.default_rng(103)
        add(f"invalid_factorisation_jacobi_{js}", options(initial_radius=1.0, jacobi_scaling=js), _pose(rng),
            Record(H_INDEFINITE, np.full(6, 0.1), 1.0, 40), [Step(_jrec(rng)), Step(_jrec(rng), rho=0.5)],
            ["begin", "invalid:solve", "idle", "candidate", "accept"], [1.0, 0.5])

    # 4. invalid by model_cost_change <= 0 although the factorisation succeeds.  With a symmetric H the change is y.(A / 2 + D).y > 0
    # for every y != 0, so: (a) an H that is not symmetric -- the identity for the factorisation, a large entry above the diagonal for
    # d.H.d -- and (b) g = 0 exactly with the gradient test switched off, where the step and the change are both zero
    rng = np.random.default_rng(104)
    H = np.eye(6); H[0, 1] = 100.0
    add("invalid_model_asymmetric", options(initial_radius=1.0, jacobi_scaling=0), _pose(rng), Record(H, np.full(6, 0.1), 1.0, 40),
        [Step(_jrec(rng)), Step(None)], ["begin", "invalid:model", "idle", "invalid:model"], [1.0, 0.5])
    add("invalid_model_zero_gradient", options(initial_radius=1.0, gradient_tolerance=-1.0), _pose(rng), _hrec(rng, g=np.zeros(6)),
        [Step(_jrec(rng)), Step(None)], ["begin", "invalid:model", "idle", "invalid:model"], [1.0, 0.5])

    # 5. invalid steps count as iterations: two of them use up max_num_iterations = 2; with 3 the third propose moves
    for n_it, third in ((2, "stop:max_iterations"), (3, "candidate")):
        rng = np.random.default_rng(105)
        add(f"invalid_counts_max_{n_it}", options(initial_radius=2.0, jacobi_scaling=0, max_num_iterations=n_it), _pose(rng),
            Record(H_INDEFINITE, np.full(6, 0.1), 1.0, 40), [Step(None), Step(None), Step(None)],
            ["begin", "invalid:solve", "invalid:solve", third], [2.0, 1.0] + ([0.5] if n_it == 3 else []))

    # 6. the stops, each followed by calls a stopped solve must ignore
    ignored = ["done"] * 5
    rng = np.random.default_rng(106)
    add("stop_gradient", r1, _pose(rng), _hrec(rng, g=np.zeros(6)), _arbitrary(rng), ["begin", "stop:gradient"] + ignored[:4])
    rng = np.random.default_rng(106)                    # a gradient that is not zero but under the tolerance (every component of
    add("stop_gradient_small", r1, _pose(rng), _hrec(rng, g=np.full(6, 2e-11)), _arbitrary(rng),   # Plus(x, -g) - x below 2e-11 sqrt(3))
        ["begin", "stop:gradient"] + ignored[:4])
    rng = np.random.default_rng(107)
    add("stop_parameter", options(initial_radius=1.0, parameter_tolerance=1e-2), _pose(rng), _hrec(rng, g=np.full(6, 1e-7)),
        [Step(_jrec(rng), cost=lambda m: m.rec.cost)] + _arbitrary(rng), ["begin", "candidate", "stop:parameter"] + ignored)
    rng = np.random.default_rng(108)
    add("stop_function", r1, _pose(rng), _jrec(rng, cost=1e8),
        [Step(_jrec(rng), cost=lambda m: m.rec.cost * (1.0 - 5e-7))] + _arbitrary(rng), ["begin", "candidate", "stop:function"] + ignored)
    rng = np.random.default_rng(109)
    add("stop_min_radius", options(initial_radius=1.0, min_radius=0.3, max_num_iterations=8), _pose(rng), _jrec(rng),
        [Step(_jrec(rng), rho=-1.0), Step(_jrec(rng), rho=-1.0)] + _arbitrary(rng),
        ["begin", "candidate", "reject", "candidate", "reject", "stop:min_radius"] + ignored[:4], [1.0, 0.5])

    # 7. the clamps.  A zero row and column 5 with g5 = 1e-9: the z step is -g5 / min_lm_diagonal at radius 1
    for mn in (1e-6, 1e-3):
        rng = np.random.default_rng(110)
        r = _jrec(rng)
        H = r.H.copy(); H[5, :] = 0.0; H[:, 5] = 0.0
        g = r.g.copy(); g[5] = 1e-9
        add(f"clamp_min_{mn:g}", options(initial_radius=1.0, min_lm_diagonal=mn), _pose(rng), Record(H, g, r.cost, 40),
            [Step(_jrec(rng), rho=0.5)], ["begin", "candidate", "accept"], [1.0])
    # max_lm_diagonal = 0.5 on a diagonal around 100: the candidate depends on the scaling; without the clamp it does not.  At 0.9
    # the clamp is on the scaled diagonal or it is not: A_ii = H_ii / (1 + sqrt(H_ii))^2 is around 0.83 here, H_ii around 100
    for mx in (0.5, 0.9, 1e32):
        for js in (1, 0):
            rng = np.random.default_rng(111)
            add(f"clamp_max_{mx:g}_jacobi_{js}", options(initial_radius=1.0, max_lm_diagonal=mx, jacobi_scaling=js), _pose(rng),
                _jrec(rng, jscale=10.0 / math.sqrt(40.0), rscale=0.1), [Step(_jrec(rng), rho=0.5)], ["begin", "candidate", "accept"], [1.0])

    # 8. the scale is computed at begin and never again: an accepted record with ten times the diagonal, max_lm_diagonal active
    rng = np.random.default_rng(112)
    add("scale_kept", options(initial_radius=1.0, max_lm_diagonal=0.5), _pose(rng), _jrec(rng, jscale=10.0 / math.sqrt(40.0), rscale=0.1),
        [Step(_jrec(rng, jscale=10.0 / math.sqrt(4.0), rscale=0.1), rho=0.5), Step(_jrec(rng), rho=0.5)],
        ["begin", "candidate", "accept", "candidate", "accept"], [1.0, 1.0])

    # 9. an infinite candidate cost is a rejection: the next round still proposes (at half the radius) and can be accepted
    rng = np.random.default_rng(113)
    add("infinite_cost", r1, _pose(rng), _jrec(rng), [Step(_jrec(rng), cost=lambda m: INF), Step(_jrec(rng), rho=0.5), Step(_jrec(rng), rho=0.5)],
        ["begin", "candidate", "reject", "candidate", "accept", "candidate", "accept"], [1.0, 0.5, 0.5])

    # 10. what follows a stop when begin is called again: after stop_min_radius (factor at 8, done set) on the same map
    rng = np.random.default_rng(114)
    add("after_restart", r1, _pose(rng), _jrec(rng), [Step(_jrec(rng), rho=-1.0), Step(_jrec(rng), rho=0.9), Step(_jrec(rng), rho=0.5)],
        ["begin", "candidate", "reject", "candidate", "accept", "candidate", "accept"], [1.0, 0.5, 0.5 / (1.0 - 0.8 ** 3)])

    # 11. the composition with the pose: a rotation step around 1 rad (a small H, the default radius), exactly zero rotation
    # components (a block-diagonal H, no rotation gradient), a start 1e3 from the origin with and without the parameter stop its
    # |x| brings about
    rng = np.random.default_rng(115)
    J = 0.05 * rng.standard_normal((40, 6))
    want = np.array([0.55, -0.6, 0.5, 0.3, -0.2, 0.1])
    add("plus_large_rotation", options(), _pose(rng), Record.from_jacobian(J, -J @ want + 1e-3 * rng.standard_normal(40)),
        [Step(_jrec(rng), rho=0.5)], ["begin", "candidate", "accept"], [1e4])
    rng = np.random.default_rng(116)
    r = _jrec(rng)
    H = r.H.copy(); H[:3, 3:] = 0.0; H[3:, :3] = 0.0
    g = r.g.copy(); g[:3] = 0.0
    add("plus_zero_rotation", r1, _pose(rng), Record(H, g, r.cost, 40), [Step(_jrec(rng), rho=0.5)], ["begin", "candidate", "accept"], [1.0])
    for name, ptol, branch in (("plus_far_start", 1e-8, "accept"), ("plus_far_start_parameter_stop", 1e-4, "stop:parameter")):
        rng = np.random.default_rng(117)
        add(name, options(initial_radius=1.0, parameter_tolerance=ptol), _pose(rng, 1e3), _jrec(rng, jscale=3.0, rscale=0.3),
            [Step(_jrec(rng), rho=0.5), Step(None)], ["begin", "candidate", branch, "candidate" if branch == "accept" else "done"])
    return out


def check_stages(sc, stages):
    """the device's pose after every call of a played scenario (Stage.got) against the policy: bit for bit wherever x is left or
    restored, an accepted pose bit for bit the candidate read after the propose before it, a candidate within candidate_bound of
    the model's.  -> the largest ratio of a candidate's error to its bound"""
    x = sc.pose0                                      # the device's x: what was set, then its own accepted candidates
    last_candidate, worst = None, 0.0
    for k, s in enumerate(stages):
        what = f"{sc.name} stage {k} ({s.call}: {s.branch})"
        if s.branch == "candidate":
            err, bound = float(np.abs(s.got - s.ref).max()), candidate_bound(s.tr, s.ref)
            worst = max(worst, err / bound)
            assert err <= bound, (what, err, bound, s.got, s.ref)
            assert not same_bits(s.got, x), what     # a candidate is a move
            last_candidate = s.got
        elif s.branch == "accept":
            assert same_bits(s.got, last_candidate), (what, s.got, last_candidate)
            x = s.got
        else:
            assert same_bits(s.got, x), (what, s.got, x)
    return worst
