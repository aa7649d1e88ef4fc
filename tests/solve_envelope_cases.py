"""Input builders and references for the tests of the Riccati pass and the line search away from the standing pose
(test_solve_envelope_cpu.py, test_gpu_solve_envelope.py).  NumPy and the CPU oracle only; no GPU.

  * tame(N=5):           the sixteen dynamics_envelope_cases.mid() states with their velocities scaled by 0.3, controls
                         grav_comp(x_i) + U(-2, 2) per knot clipped to 0.9 ctrlrange, physical gravity, h = 0.02 unless `h` is given; the trajectory is the
                         oracle's ROLLOUT of those controls, so every knot is another linearisation point.  On these lxx is indefinite,
                         and some rollouts reach the `indefinite even after the +1e-4 bump' branch of the Riccati pass at some knot.
  * tame_contact(mode):  the same states and controls (first four knots), contact mode 1 or 2 under dynamics_envelope_cases.SCHEDULE.
  * SCALES:              factors on lx and lu only.  K, Vxx and the branches stay, kff and Vx scale, and the candidate of (scale s,
                         slot alpha) is the candidate of (1, s alpha): the same physics is accepted through another alpha slot.
  * bumped_luu():        natural data never lands in the 1e-4 wide window of the `bumped' branch (LLT fails, passes after +1e-4): the
                         diagonal of luu at ONE knot of a rollout with an indefinite knot is shifted so that it does; everything else,
                         the indefinite lxx and the fold products among it, stays natural.
  * riccati_ref():       ilqr.cpp:250-309 in a chosen floating-point type (np.longdouble: the reference; np.float64: its spread), with
                         the branch every knot took and the pivot that decided it.
  * candidates_ref():    the eight candidates of ilqr.cpp:311-361 by the oracle's step and total cost, the accept decision, its margins.
  * mutants of both:     the slips a kernel could make (RICCATI_MUTANTS, LS_MUTANTS); test_solve_envelope_cpu.py shows that the inputs see
                         every one of them at a hundred times the tolerance of the GPU test."""
import functools
import hashlib

import numpy as np

import dynamics_envelope_cases as dc
import oracle_lib as ol

NS, NX, NU, NQ = dc.NS, dc.NX, dc.NU, dc.NQ
LD = np.longdouble
SEED = 7
LAMBDA = 1e-6
ALPHAS = (1.0, 0.8, 0.6, 0.4, 0.2, 0.1, 0.05, 0.01)
SCALES = (1, 4, 16)
BUMP = 1e-4                                  # ilqr.cpp:278: Quu += 1e-4 I after a failed LLT
ACCEPT = 1e-6                                # ilqr.cpp:349: accepted if cost < baseline - 1e-6
# tolerances of the GPU test: the project's own (riccati_golden `spd' / `bump' and the folded test; the standing-pose line-search test)
TOL_SPD, TOL_BUMPED = 1e-9, 1e-6
TOL_COST, TOL_X, TOL_U = 1e-8, 1e-8, 1e-7
PIVOT_DECISIVE = 1e-6                        # |deciding pivot| / largest diagonal entry of Quu
MARGIN_DECISIVE = 1e-4                       # |candidate cost - (baseline - 1e-6)| / |baseline|
MAX_DROPPED = 2
BUMPED_EIG = -5e-5                           # bumped_luu(): the smallest eigenvalue of Quu it leaves, half-way into (-1e-4, 0)
RICCATI_MUTANTS = ("no_quat_rows", "no_lambda", "no_bump")
LS_MUTANTS = ("drop_K_col50", "drop_quat_dx", "alpha_shift")
# the steps of dc.TIMESTEPS at which the line search is tested: at 0.04 fifteen of the 48 free-flight cases are undecided (test_timestep_cpu.py)
LS_TIMESTEPS = dc.TIMESTEPS[:2]
LS_WIDE_SCALE = 1                            # the scale of the four-rollouts-per-wave case at LS_TIMESTEPS[0]: five alpha slots are accepted there (three at scale 4)
SOLVE_B, SOLVE_N, SOLVE_SEED, SOLVE_ITERATIONS = 4, 8, 31, 5       # standing_solve(): one full solve per time step


def rel(a, b):
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# trajectories
def oracle_of(prob, mode=0, **opts):
    """an oracle of the problem; .stance_rows: the schedule its contact-mode steps run under, knot by knot (None: constraint-free)"""
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(prob); o.set_contact_mode(mode); o.set_options(lam=LAMBDA, **opts)
    o.stance_rows = np.array(o._keep[3]).reshape(-1, 2) if mode else None
    return o


@functools.lru_cache(maxsize=None)
def tame(N=5, mode=0, h=dc.H):
    """(prob, X [16,N+1,51], U [16,N,19]); read-only.  mode != 0: N = 4 under dc.SCHEDULE.  prob["dt"] = h: the rollout steps by it"""
    x = dc.mid()[0].copy()
    x[:, NQ:] *= 0.3
    prob = dc.problem(N, dc.SCHEDULE if mode else None, h=h)
    o = oracle_of(prob, mode)
    noise = np.random.default_rng(SEED).uniform(-2.0, 2.0, (NS, 5, NU))
    lim = 0.9 * dc.sc.CTRLRANGE
    X, U = np.zeros((NS, N + 1, NX)), np.zeros((NS, N, NU))
    for i in range(NS):
        U[i] = np.clip(o.grav_comp(x[i])[None] + noise[i, :N], -lim, lim)
        o.initialize(x[i], U[i])
        X[i] = o.get("xbar")
        assert np.array_equal(o.get("ubar"), U[i])
    X.setflags(write=False); U.setflags(write=False)
    return prob, X, U


def tame_contact(mode, h=dc.H):
    return tame(4, mode, h)


def trajectories(name, h=dc.H):
    """name: "tame", "contact1", "contact2" -> (prob, mode, X, U)"""
    mode = 0 if name == "tame" else int(name[-1])
    prob, X, U = tame(5, 0, h) if mode == 0 else tame_contact(mode, h)
    return prob, mode, X, U


@functools.lru_cache(maxsize=None)
def oracle_inputs(name, h=dc.H):
    """the oracle's own Jacobians (forward-mode AD) and cost quadratics along the trajectories: dict of arrays over the sixteen rollouts;
    read-only.  (The GPU test hands the DEVICE's to the references; these serve the CPU test.)"""
    prob, mode, X, U = trajectories(name, h)
    o = oracle_of(prob, mode)
    out = {k: [] for k in ("A", "B", "lx", "lu", "lxx", "luu")}
    for i in range(NS):
        o.set_trajectory(X[i], U[i]); o.linearize(); o.cost_quadratics()
        for k in out:
            out[k].append(o.get(k))
    out = {k: np.array(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def scaled(lx, lu, s):
    return lx * float(s), lu * float(s)


def standing_solve(h=dc.H):
    """(prob, x0 [4,51], u_init [4,8,19]): the shipped problem (its own gravity) with prob["dt"] = h over N = 8, and the seeded perturbed
    standing batch about the oracle's gravity compensation"""
    prob = dc.sc.make_problem(ol.reference_kinematics, N=SOLVE_N)
    prob["dt"] = float(h)
    o = ol.Oracle(SOLVE_N, h); o.set_problem(prob)
    x0, ui = dc.sc.synthetic_batch(SOLVE_B, SOLVE_N, SOLVE_SEED, o.grav_comp(dc.sc.standing_state()))
    return prob, x0, ui


def standing_solve_ref(prob, x0, ui):
    """the oracle's cold solve of one rollout (five iterations at the most, default options) and its warm-started second solve from the
    same x0 (the first solution shifted by one knot): two dicts with it, cost [6], alpha [5], lam [5], K, xbar, ubar, final cost"""
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(prob); o.set_options(max_iter=SOLVE_ITERATIONS)
    out = []
    for warm in (False, True):
        if warm:
            o.initialize(x0, None, out[0]["xbar"], out[0]["ubar"])
        else:
            o.initialize(x0, ui)
        _, c = o.solve(x0)
        it, cost, alpha, lam = o.trace()
        out.append(dict(it=it, cost=cost, alpha=alpha, lam=lam, K=o.get("K"), xbar=o.get("xbar"), ubar=o.get("ubar"), final=c))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# Riccati pass
def _cholesky(Q, dtype):
    """(L, smallest pivot) -- or (None, the pivot that was not positive): Eigen::LLT's NumericalIssue"""
    m = Q.shape[0]
    L = np.zeros((m, m), dtype)
    smallest = dtype(np.inf)
    for j in range(m):
        s = Q[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not s > 0:
            return None, s
        smallest = min(smallest, s)
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (Q[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, smallest


def _cholesky_solve(L, R, dtype):
    m = L.shape[0]
    Y = np.zeros(R.shape, dtype)
    for i in range(m):
        Y[i] = (R[i] - L[i, :i] @ Y[:i]) / L[i, i]
    Z = np.zeros(R.shape, dtype)
    for i in range(m - 1, -1, -1):
        Z[i] = (Y[i] - L[i + 1:, i] @ Z[i + 1:]) / L[i, i]
    return Z


def _pivoted_solve(Q, R, dtype):
    """(Q^-1 R, smallest |pivot|) by elimination with partial pivoting: the symmetric indefinite system the reference hands to ldlt()"""
    m = Q.shape[0]
    M = np.concatenate([Q, R], axis=1).astype(dtype)
    smallest = dtype(np.inf)
    for c in range(m):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, p]] = M[[p, c]]
        smallest = min(smallest, abs(M[c, c]))
        M[c] = M[c] / M[c, c]
        for r in range(m):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, m:], smallest


def riccati_ref(A, B, lx, lu, lxx, luu, lam=LAMBDA, dtype=LD, mutant=None):
    """ilqr.cpp:250-309 for one rollout in `dtype` (as test_gpu_configs._riccati_numpy states it, with the LLT-failure rule spelled out:
    +1e-4 on the diagonal, and if LLT fails again, elimination with partial pivoting on the bumped matrix).  Returns a dict: K [N,19,51],
    k [N,19], Vx [51], Vxx [51,51] in `dtype`; branch [N] (0 Cholesky, 1 bumped, 2 indefinite); pivot [N], of the factorisations the
    knot's decision rests on the pivot of smallest magnitude (a passing LLT: its smallest pivot; a failing one: the pivot that was not
    positive) divided by the largest diagonal entry of that Quu; ge_pivot [N], the smallest |pivot| of the elimination (branch 2);
    eig [N], the smallest eigenvalue of Quu + lambda I before any bump (fp64 eigvalsh); diag [N], its largest diagonal entry."""
    assert mutant is None or mutant in RICCATI_MUTANTS
    A, B, lx, lu, lxx, luu = [np.asarray(a).astype(dtype) for a in (A, B, lx, lu, lxx, luu)]
    N, n, m = A.shape[0], A.shape[1], B.shape[2]
    eye = np.eye(m, dtype=dtype)
    lam = dtype(0.0 if mutant == "no_lambda" else lam)
    Vx, Vxx = lx[N].copy(), lxx[N].copy()
    K, k = np.zeros((N, m, n), dtype), np.zeros((N, m), dtype)
    branch, pivot, ge_pivot = np.zeros(N, dtype=int), np.zeros(N), np.full(N, np.nan)
    eig, diag = np.zeros(N), np.zeros(N)
    for t in range(N - 1, -1, -1):
        At, Bt = A[t], B[t]
        Ap = At
        if mutant == "no_quat_rows":                          # the quaternion rows of A_t left out of the Vxx products
            Ap = At.copy(); Ap[3:7] = 0
        Qx = lx[t] + At.T @ Vx; Qu = lu[t] + Bt.T @ Vx
        Qxx = lxx[t] + Ap.T @ Vxx @ Ap
        Quu = np.diag(luu[t]) + Bt.T @ Vxx @ Bt + lam * eye
        Qxu = Ap.T @ Vxx @ Bt
        R = np.concatenate([Qxu.T, Qu[:, None]], axis=1)
        scale = np.abs(np.diag(Quu)).max()
        eig[t], diag[t] = np.linalg.eigvalsh(Quu.astype(np.float64)).min(), float(scale)
        L, p = _cholesky(Quu, dtype)
        piv = [p]
        if L is None:
            branch[t] = 1
            if mutant != "no_bump":
                Quu = Quu + dtype(BUMP) * eye
            L, p = _cholesky(Quu, dtype)
            piv.append(p)
        if L is None:
            branch[t] = 2
            Z, g = _pivoted_solve(Quu, R, dtype)
            ge_pivot[t] = float(g)
        else:
            Z = _cholesky_solve(L, R, dtype)
        pivot[t] = float(min(piv, key=abs) / scale)
        K[t] = -Z[:, :n]; k[t] = -Z[:, n]
        Vx = Qx + K[t].T @ Quu @ k[t] + K[t].T @ Qu + Qxu @ k[t]
        Vxx = Qxx + K[t].T @ Quu @ K[t] + K[t].T @ Qxu.T + Qxu @ K[t]
        Vxx = (Vxx + Vxx.T) / 2
    return dict(K=K, k=k, Vx=Vx, Vxx=Vxx, branch=branch, pivot=pivot, ge_pivot=ge_pivot, eig=eig, diag=diag)


def bumped_luu(luu, ref):
    """luu [N,19] of a rollout with a knot on branch 2, with the diagonal at the last such knot (the first one the recursion meets, so
    everything before it is unchanged) shifted uniformly so that the smallest eigenvalue of its Quu becomes BUMPED_EIG: the LLT fails
    and passes after the +1e-4 bump.  `ref`: riccati_ref() of the unshifted inputs.  None for a rollout without such a knot."""
    t = np.flatnonzero(ref["branch"] == 2)
    if not len(t):
        return None
    out = np.array(luu, dtype=np.float64)
    out[t.max()] += BUMPED_EIG - ref["eig"][t.max()]
    return out


RICCATI_KEYS = ("K", "k", "Vx", "Vxx")
_ref_cache = {}


def riccati_ref_cached(A, B, lx, lu, lxx, luu, dtype=LD):
    """riccati_ref(lambda = LAMBDA, no mutant), remembered by the bytes of its inputs (kernel families are run on the same inputs)"""
    h = hashlib.sha1()
    for a in (A, B, lx, lu, lxx, luu):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    key = (h.hexdigest(), np.dtype(dtype).name)
    if key not in _ref_cache:
        _ref_cache[key] = riccati_ref(A, B, lx, lu, lxx, luu, LAMBDA, dtype)
    return _ref_cache[key]


def riccati_tol(branch):
    """the project's own: 1e-9 max(1, max |want|) where every knot factorised (the `spd' golden), 1e-6 with a bumped or indefinite knot
    (the `bump' golden, the folded test)"""
    return TOL_SPD if np.all(np.asarray(branch) == 0) else TOL_BUMPED


def riccati_error(got, want):
    """max |got - want| / max(1, max |want|): the figure the tolerances bound"""
    want = np.asarray(want)
    return float(np.abs(np.asarray(got) - want).max() / max(1.0, float(np.abs(want).max())))


def branches_decisive(ref_ld, ref_64=None):
    """no factorisation of the rollout was decided by a pivot below 1e-6 of the largest diagonal entry -- nor by a smallest eigenvalue
    (of Quu, and of the bumped Quu where the first LLT failed) within 1e-6 of it of zero -- and fp64 takes the same branches"""
    ok = bool(np.all(np.abs(ref_ld["pivot"]) >= PIVOT_DECISIVE))
    ok = ok and bool(np.all(np.abs(ref_ld["eig"]) >= PIVOT_DECISIVE * ref_ld["diag"]))
    ok = ok and bool(np.all((np.abs(ref_ld["eig"] + BUMP) >= PIVOT_DECISIVE * ref_ld["diag"]) | (ref_ld["branch"] == 0)))
    if ref_64 is not None:
        ok = ok and np.array_equal(ref_ld["branch"], ref_64["branch"])
    return ok


# ---------------------------------------------------------------------------------------------------------------------------------------
# line search
def candidates_ref(o, xb, ub, K, k, mutant=None):
    """ilqr.cpp:311-361 for one rollout by the oracle `o` (of oracle_of(): problem, contact mode and schedule set): dict with X [8,N+1,51], U [8,N,19],
    cost [8] of the eight candidates, baseline, slot (the accepted one, -1: none), alpha (ALPHAS[slot], 0.0: none), margin [8] =
    |cost - (baseline - 1e-6)| / |baseline|, and decisive: every candidate up to and including the accepted one (all eight of a
    rejection) has a margin of at least 1e-4.  Leaves (xb, ub) as the oracle's trajectory."""
    assert mutant is None or mutant in LS_MUTANTS
    N = ub.shape[0]
    K = np.array(K, dtype=np.float64); k = np.asarray(k, dtype=np.float64)
    stance = o.stance_rows
    alphas = ALPHAS[1:] + (ALPHAS[-1] / 2,) if mutant == "alpha_shift" else ALPHAS          # slot i steps by the next slot's alpha
    if mutant == "drop_K_col50":
        K[:, :, 50] = 0.0
    o.set_trajectory(xb, ub)
    baseline = o.total_cost()
    X, U, cost = np.zeros((8, N + 1, NX)), np.zeros((8, N, NU)), np.zeros(8)
    for a, alpha in enumerate(alphas):
        X[a, 0] = xb[0]
        for t in range(N):
            dx = X[a, t] - xb[t]
            if mutant == "drop_quat_dx":
                dx[3:7] = 0.0
            U[a, t] = ub[t] + alpha * k[t] + K[t] @ dx
            X[a, t + 1] = o.step(X[a, t], U[a, t]) if stance is None else o.step_stance(X[a, t], U[a, t], stance[t])
        o.set_trajectory(X[a], U[a])
        cost[a] = o.total_cost()
    o.set_trajectory(xb, ub)
    ok = np.flatnonzero(cost < baseline - ACCEPT)
    slot = int(ok[0]) if len(ok) else -1
    margin = np.abs(cost - (baseline - ACCEPT)) / abs(baseline)
    decisive = bool(np.all(margin[: slot + 1 if slot >= 0 else 8] >= MARGIN_DECISIVE))
    return dict(X=X, U=U, cost=cost, baseline=baseline, slot=slot, alpha=ALPHAS[slot] if slot >= 0 else 0.0, margin=margin, decisive=decisive)


def accepted(c):
    """(cost, xbar, ubar) the line search leaves behind: the accepted candidate, or the baseline and None, None"""
    return (c["cost"][c["slot"]], c["X"][c["slot"]], c["U"][c["slot"]]) if c["slot"] >= 0 else (c["baseline"], None, None)
