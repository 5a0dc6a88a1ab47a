"""The inputs of tests/test_gpu_pl.py, generated from seeds: one ``Case`` per launch of ace_pl_host.  Kept apart from
the GPU tests so that tests/test_pl_ref.py can run its wrong-kernel models on exactly these inputs without a GPU.

Every launch is given every array of the entry with random contents (so a buffer the operation must not touch has
something to lose) and a state whose unused fields hold distinct non-zero values.  Shapes: d over both sides of
d^2 = 256, 512, 768 (the copy loop of pl_outer_begin_kernel) and of every 32-tile tail, m over the 256-thread
strides; batches of 5 to 7 mix done, inactive and every reachable flag combination in one launch."""
from __future__ import annotations

import dataclasses

import numpy as np

import pl_ref as R

DS = (1, 2, 16, 17, 23, 28, 31, 32, 33, 64, 65, 96)
MS = (1, 40, 255, 256, 257, 513)
DM = ((1, 2), (2, 40), (16, 255), (17, 256), (23, 257), (33, 513))   # m > d: apply_a, grad, gy
POISON = 3.0e150   # large and finite: a product with it survives as something huge, not as NaN


@dataclasses.dataclass
class Case:
    op: str
    id: str
    batch: int
    m: int
    d: int
    A: dict
    S: np.ndarray
    p: dict
    reduced: int = 0


def shapes(batch, m, d):
    """name -> (shape, dtype) of every array of the entry (ace_amd.plstep.shapes restated)."""
    c, f, i = np.complex128, np.float64, np.int32
    s = {k: ((batch, d, d), c) for k in ("x", "xo", "z", "zo", "y", "G", "Znew", "P", "VT", "V", "C")}
    s.update({k: ((batch, m), f) for k in ("Ax", "Axo", "Az", "Azo", "Ay", "gAy", "gAx", "Aex", "bvec")})
    s.update(R=((d, m), c), RT=((m, d), c), Pg=((batch, d, m), c), T=((batch, d, m), c), tau=((batch,), f),
             lam=((batch, d), f), misc=((batch, 3), f), K=((m, m), c), cholR=((m, m), c), V1=((batch, d), c),
             w=((batch, d), c), act=((batch,), i), cnt=((9,), i), ok=((1,), i), iters=((batch,), i),
             status=((batch,), i))
    return s


def rng_of(*key):
    return np.random.default_rng([int(k) for k in key])


def arrays(rng, batch, m, d):
    A = {}
    for k, (shape, dt) in shapes(batch, m, d).items():
        if dt == np.complex128:
            A[k] = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        elif dt == np.float64:
            A[k] = rng.standard_normal(shape)
        else:
            A[k] = rng.integers(1, 50, shape).astype(np.int32)
    A["act"][:] = 1
    A["tau"] = np.abs(A["tau"]) + 0.1
    A["misc"][:] = 0.0
    return A


DEFAULT = dict(L=1.3, L_old=1.0, theta=0.6, theta_old=0.8, f_x=2.5, f_y=2.25, C_x=0.1, C_z=0.2, cntr_Ax=1.0,
               cntr_Ay=2.0, xy_sq=0.5, nx2=4.0, ndx2=0.25, dot_xy_g=0.125, localL=1.1, step=0.7, n_iter=3,
               restart_iter=0, backtrack_simple=1, backtrack_steps=0, have_gAy=1, have_gy=1, have_gAx=1, ycomp=1,
               need_Ay=0, need_Ax=0, inner=1, done=0, status=0)


def state(batch, rows=None, **cols):
    """[batch][len(STATE)]: DEFAULT, then whole columns (cols), then per-realisation overrides (rows: list of dicts)."""
    S = np.zeros((batch, len(R.STATE)))
    for k, v in {**DEFAULT, **cols}.items():
        S[:, R.IX[k]] = v
    for b, r in enumerate(rows or []):
        for k, v in r.items():
            S[b, R.IX[k]] = v
    return S


def _case(op, tag, batch, m, d, S=None, p=None, seed=0, **over):
    rng = rng_of(R.IX["theta"] + list(R.OPS).index(op) if op in R.OPS else 99, batch, m, d, seed)
    A = arrays(rng, batch, m, d)
    reduced = over.pop("reduced", 0)
    A.update(over)
    return Case(op, f"{op}-{tag}-b{batch}-m{m}-d{d}", batch, m, d, A, state(batch) if S is None else S,
                R.params(**(p or {})), reduced)


# ------------------------------------------------------------------------------------------ element-wise and copies
def init_cases():
    return [_case("init", "m", 3, m, 2) for m in MS]


def outer_begin_cases():
    out = []
    for d in DS:
        m = {1: 1, 33: 257, 96: 513}.get(d, 40)
        out.append(_case("outer_begin", "tails", 5, m, d, state(5, done=[0, 1, 0, 0, 1], inner=[0, 0, 1, 0, 0],
                                                                  L=[1.3, 1.3, 0.7, 1e-3, 5.0], theta=[np.inf, 0.5, 0.6, 1.0, 0.2])))
    return out


def theta_cases():
    out = []
    for batch, reset, seed in ((257, 3, 0), (6, 50, 1)):
        rng = rng_of(7, batch, reset)
        S = state(batch, inner=rng.integers(0, 2, batch), done=rng.integers(0, 4, batch) == 0,
                  theta_old=np.where(rng.integers(0, 4, batch) == 0, np.inf, rng.uniform(0.05, 1.0, batch)),
                  L=np.where(rng.integers(0, 2, batch) == 0, 0.9, rng.uniform(1.0, 4.0, batch)),
                  cntr_Ay=rng.choice([0.0, reset - 1.0, float(reset), reset + 1.0, np.inf], batch),
                  have_gAy=rng.integers(0, 2, batch), ycomp=rng.integers(0, 2, batch), need_Ay=rng.integers(0, 2, batch))
        S[:, R.IX["have_gy"]] = S[:, R.IX["have_gAy"]] * rng.integers(0, 2, batch)   # (have_gy without g_Ay: unreachable)
        c = _case("theta", f"reset{reset}", batch, 1, 2, S, dict(cntr_reset=reset), seed)
        c.A["cnt"][:] = np.arange(9) + 3
        out.append(c)
    return out


def _mixed(batch):
    """act / ycomp / need_Ay / need_Ax / theta mixed over a batch of 6: inactive, theta = 1, combinations, exact."""
    assert batch == 6
    act = np.array([1, 0, 1, 1, 1, 1], np.int32)
    S = state(6, ycomp=[1, 1, 0, 1, 1, 1], need_Ay=[0, 1, 0, 1, 0, 1], need_Ax=[0, 1, 1, 1, 0, 0],
              theta=[0.6, 0.5, 1.0, 0.37, 0.999, 1e-3])
    return act, S


def make_y_cases():
    act, S = _mixed(6)
    return [_case("make_y", "mix", 6, 3, d, S, act=act) for d in DS]


def set_ay_cases():
    act, S = _mixed(6)
    return [_case("set_ay", "mix", 6, m, 2, S, act=act) for m in MS]


def set_ax_cases():
    act, S = _mixed(6)
    return [_case("set_ax", "mix", 6, m, 2, S, act=act) for m in MS]


def grad_cases():
    out = []
    for d, m in ((1, 1),) + DM:
        act = np.array([1, 1, 1, 0, 1, 1], np.int32)
        # (have_gAy, have_gy): fresh y (0, 0), restart with g_Ax (1, 0), nothing stale (1, 1), inactive
        S = state(6, have_gAy=[0, 1, 1, 0, 0, 1], have_gy=[0, 0, 1, 0, 0, 0], theta=[0.6, 1.0, 0.3, 0.5, 0.01, 1.0],
                  L=[1.3, 1.0, 7.0, 1.0, 1e3, 0.9])
        out.append(_case("grad", "mix", 6, m, d, S, dict(lam_reg=5e-2), act=act))
    return out


def gy_cases():
    return [_case("gy", "mgtd", 3, m, d) for d, m in DM]


def apply_a_cases():
    return [_case("apply_a", "mgtd", 5, m, d, act=np.array([1, 0, 1, 1, 0], np.int32)) for d, m in DM]


def prox_in_cases():
    return [_case("prox_in", "tiles", 3, 2, d, state(3, step=[0.7, 0.3, 11.0]), act=np.array([1, 0, 1], np.int32))
            for d in DS]


def transpose_cases():
    return [_case("transpose", "rc", 1, m, d) for d, m in ((1, 1), (31, 33), (33, 31), (32, 64), (65, 40), (2, 513))]


def outputs_cases():
    out = []
    for batch in (257, 5):
        rng = rng_of(11, batch)
        c = _case("outputs", "all", batch, 1, 2, state(batch, status=rng.integers(0, 5, batch),
                                                       n_iter=rng.integers(1, 4000, batch)))
        c.A["status"] = (rng.integers(0, 4, batch) * 2).astype(np.int32)   # other ACE_ST_* bits already set
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------- make_x
def make_x_cases():
    out = []
    for d in DS:
        m = {1: 1, 33: 257, 96: 513}.get(d, 40)
        reset = 3
        act = np.array([1, 0, 1, 1, 1, 1, 1], np.int32)
        S = state(7, ycomp=[1, 1, 0, 1, 1, 1, 1], theta=[0.6, 0.5, 1.0, 0.37, 0.999, 0.25, 0.5],
                  cntr_Ax=[0.0, 0.0, 5.0, float(reset), reset - 1.0, np.inf, reset + 1.0], C_z=0.375)
        c = _case("make_x", "mix", 7, m, d, S, dict(cntr_reset=reset), act=act)
        c.A["cnt"][:] = np.arange(9) + 1
        # realisation 4: x close to y (a small ||x - y||^2 from cancelling entries)
        c.A["y"][4] = (1 - 0.999) * c.A["xo"][4] + 0.999 * c.A["z"][4] + 1e-9 * c.A["y"][4]
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------- backtrack
def _f_x(Ax, b):
    g = (Ax - b).astype(R.LD)
    return float(0.5 * (g * g).sum())


def backtrack_cases():
    out = []
    for m in (1, 40, 257):
        # (a) simple: break, growth (finite), growth (Inf), xy_sq == 0, inactive, forced reset, flip to non-simple
        rng = rng_of(21, m)
        B = 7
        A = arrays(rng, B, m, 2)
        L, xy = 1.5, 0.25
        fx = np.array([_f_x(A["Ax"][b], A["bvec"][b]) for b in range(B)])
        rows = [dict(f_y=fx[0] * 1.3, dot_xy_g=0.0),                                   # f_x < q_x: localL = L, break
                dict(f_y=fx[1] - 0.5 * L * xy - 1.5 * L * xy, dot_xy_g=0.0),           # localL = 4 L -> L = 8 L
                dict(f_y=fx[2] * 0.25, dot_xy_g=0.0, xy_sq=1e-320, nx2=1e-310),        # quotient overflows: localL = Inf
                dict(xy_sq=0.0),                                                       # do_break
                dict(),                                                                # inactive
                dict(f_y=fx[5] * 1.3, dot_xy_g=0.0, xy_sq=1e-20, nx2=1e4, cntr_Ax=7.0),  # xy_sq / nx2 < eps
                dict(f_y=fx[6] * (1 + 1e-12), dot_xy_g=-1.0 - fx[6])]                  # |f_y - f_x| < 1e-10 max: flips
        S = state(B, rows, L=L, xy_sq=xy, backtrack_steps=[0, 1, 2, 0, 0, 0, 0])
        A["act"][:] = [1, 1, 1, 1, 0, 1, 1]
        out.append(Case("backtrack", f"backtrack-simple-b{B}-m{m}-d2", B, m, 2, A, S, R.params(beta=0.5)))
        # (b) non-simple: break and growth; (c) simple with beta = 0.25
        A = arrays(rng, B, m, 2)
        e = rng.standard_normal((B, m))
        A["Ay"] = A["Ax"] - e
        A["gAy"] = (A["Ax"] - A["bvec"]) - 2.0 * e      # <A_x - A_y, g_Ax - g_Ay> = 2 ||e||^2
        ee = (e * e).sum(axis=1)
        rows = [dict(backtrack_simple=0, xy_sq=4 * ee[0] / (0.5 * L)),                 # localL = L / 2: break
                dict(backtrack_simple=0, xy_sq=4 * ee[1] / (3 * L)),                   # localL = 3 L -> L = 6 L
                dict(backtrack_simple=0, xy_sq=4 * ee[2] / (3 * L), have_gAx=0, cntr_Ax=2.0),
                dict(backtrack_simple=0, xy_sq=0.0, have_gAx=0),
                dict(backtrack_simple=0, have_gAx=0),                                  # inactive
                dict(backtrack_simple=0, xy_sq=4 * ee[5] / (0.9 * L), have_gAx=0),
                dict(backtrack_simple=1, f_y=_f_x(A["Ax"][6], A["bvec"][6]) - 1.0, dot_xy_g=0.0, xy_sq=0.5)]
        S = state(B, rows, L=L, nx2=1e3)
        A["act"][:] = [1, 1, 1, 1, 0, 1, 1]
        out.append(Case("backtrack", f"backtrack-nonsimple-b{B}-m{m}-d2", B, m, 2, A, S, R.params(beta=0.5)))
        # (d) a finite Lexact: L == Lexact (the tie) and L > Lexact stop the growth; localL beyond Lexact is clamped
        A = arrays(rng, 5, m, 2)
        fx = np.array([_f_x(A["Ax"][b], A["bvec"][b]) for b in range(5)])
        rows = [dict(L=3.0, f_y=fx[0] - 10.0, dot_xy_g=0.0),      # localL > L but L >= Lexact: break, L kept
                dict(L=3.5, f_y=fx[1] - 10.0, dot_xy_g=0.0),
                dict(L=1.5, f_y=fx[2] - 10.0, dot_xy_g=0.0),      # localL = 1.5 + 80 -> min(Lexact, .) = 3
                dict(L=1.0, f_y=fx[3] - 0.125 - 0.5 * 0.25, dot_xy_g=0.0),   # localL = 2 -> L = min(3, 2 / beta) = 3
                dict(L=0.5, f_y=fx[4] - 0.5 * 0.5 * 0.25 - 0.03125, dot_xy_g=0.0)]  # localL = 0.75 -> L = 1.5
        out.append(Case("backtrack", f"backtrack-lexact-b5-m{m}-d2", 5, m, 2, A, state(5, rows, xy_sq=0.25),
                        R.params(beta=0.5, Lexact=3.0)))
    return out


# ------------------------------------------------------------------------------------------------------ iterate
def iterate_cases():
    out = []
    p = dict(tol=2.0 ** -10, maxIts=10, restart=4)
    for d, m in ((2, 40), (17, 257), (33, 1)):
        rows = [dict(f_y=np.nan),                                         # NaN: stop 1
                dict(ndx2=0.0, n_iter=2),                                 # ||dx|| = 0: stop 1
                dict(ndx2=0.0, n_iter=0, backtrack_steps=2),              # ... at the first iteration: goes on
                dict(ndx2=1e-8, nx2=4.0),                                 # 1e-4 < 2^-10 * 2: stop 2
                dict(n_iter=9, ndx2=1.0),                                 # n_iter == maxIts: stop 3
                dict(done=1, status=2, n_iter=5, restart_iter=1),         # done: untouched
                dict(n_iter=5, restart_iter=4, ndx2=1.0, backtrack_steps=3)]   # plain: no stop, no restart
        c = _case("iterate", "stops", 7, m, d, state(7, rows, have_gAy=0), p)
        c.A["cnt"][:] = [1, 2, 3, 4, 5, 6, 7, 8, 2]
        out.append(c)
        rows = [dict(backtrack_steps=1, xy_sq=0.0, ndx2=1.0),             # stop 4
                dict(n_iter=7, restart_iter=4, ndx2=1.0, have_gAx=1, have_gAy=0, backtrack_simple=0, f_x=1.75),
                dict(n_iter=3, restart_iter=0, ndx2=1.0, have_gAx=0, have_gAy=1, backtrack_simple=0, f_x=np.inf),
                dict(done=1, status=3, n_iter=7, restart_iter=4),         # done at a restart point: untouched
                dict(n_iter=9, restart_iter=6, ndx2=1.0),                 # maxIts and restart together: stop 3
                dict(ndx2=2.0 ** -18, nx2=4.0, n_iter=3, restart_iter=0),     # norm_dx == tol * norm_x exactly: not <; restart
                dict(ndx2=1e-7, nx2=1e-4)]                                # max(norm_x, 1) = 1: 3.2e-4 < 2^-10: stop 2
        c = _case("iterate", "restart", 7, m, d, state(7, rows), p, seed=1)
        c.A["cnt"][:] = 0
        out.append(c)
    return out


# ----------------------------------------------------------------------------------------- assemble, zasm, take_z
def prox_cases(d, flip=0):
    """One realisation per kept count k in {0, 1, 31, 32, 33, d} (those <= d), sides alternating (flip swaps them)."""
    ks = sorted({k for k in (0, 1, 31, 32, 33, d) if k <= d})
    while len(ks) < 5:
        ks.append(ks[-1])
    ks.append(ks[1])   # (inactive)
    B = len(ks)
    side = (np.arange(B) + flip) % 2
    rng = rng_of(31, d, flip)
    A = arrays(rng, B, 2, d)
    A["misc"] = np.stack([np.array(ks, float), rng.uniform(0.5, 2.0, B), side.astype(float)], axis=1)
    A["act"][:] = 1
    A["act"][B - 1] = 0
    A["P"][:] = POISON * (1 + 1j)
    A["VT"][:] = POISON * (1 - 1j)
    S = state(B, step=rng.uniform(0.2, 2.0, B))
    return ks, A, S


def assemble_cases():
    out = []
    for d in (1, 2, 31, 32, 33, 64, 65, 96):
        for flip in (0, 1):
            ks, A, S = prox_cases(d, flip)
            out.append(Case("assemble", f"assemble-k-b{len(ks)}-d{d}-f{flip}", len(ks), 2, d, A, S, R.params()))
    return out


def zasm_cases():
    """VT and P as pl_assemble leaves them on poisoned buffers: columns q < k random, k <= q < 32 ceil(k / 32) zero,
    the rest poison."""
    out = []
    for d in (1, 2, 31, 32, 33, 64, 65, 96):
        ks, A, S = prox_cases(d, 0)
        for b, k in enumerate(ks):
            kw = min(d, 32 * ((k + 31) // 32))
            for name in ("P", "VT"):
                A[name][b][:, :k] = A["Znew"][b][:, :k] if name == "P" else A["V"][b][:, :k]
                A[name][b][:, k:kw] = 0.0
        out.append(Case("zasm", f"zasm-k-b{len(ks)}-d{d}", len(ks), 2, d, A, S, R.params()))
    return out


def take_z_cases():
    out = []
    for d in (1, 2, 31, 32, 33, 64, 65, 96):
        for flip in (0, 1):
            ks, A, S = prox_cases(d, flip)
            out.append(Case("take_z", f"take_z-b{len(ks)}-d{d}-f{flip}", len(ks), 2, d, A, S, R.params()))
    return out


# ---------------------------------------------------------------------------------------------- chol, final_vec
def chol_matrices(m, kind, seed=0):
    rng = rng_of(41, m, seed)
    X = rng.standard_normal((m, m + 3)) + 1j * rng.standard_normal((m, m + 3))
    K = X @ X.conj().T / (m + 3) + np.eye(m)
    if kind == "graded":
        s = np.exp2(-30.0 * np.arange(m) / max(m - 1, 1))
        K = K * s[:, None] * s[None, :]
    elif kind == "indefinite":
        K[m // 2, m // 2] = -1.0
    elif kind == "singular":   # a leading block [[4, 2], [2, 1]] uncoupled from the rest: the second pivot is 1 - 1 = 0 exactly
        K[:2, :] = 0.0
        K[:, :2] = 0.0
        K[:2, :2] = [[4.0, 2.0], [2.0, 1.0]]
    K = 0.5 * (K + K.conj().T)
    return np.ascontiguousarray(K)


def chol_cases():
    out = []
    for m, kind in [(m, "well") for m in (1, 2, 17, 40, 255, 257)] + [(40, "graded"), (257, "graded"),
                                                                       (17, "indefinite"), (33, "singular")]:
        out.append(_case("chol", kind, 1, m, 1, K=chol_matrices(m, kind)))
    return out


def final_vec_cases():
    out = []
    for d in (1, 2, 33, 257):
        for reduced in (1, 0):
            rng = rng_of(51, d, reduced)
            B = 5
            m = d if reduced else max(d - 1, 1)
            A = arrays(rng, B, m, d)
            A["lam"][:, 0] = [2.5, 0.0, -1.25, 1e-12, 0.7]
            if reduced:
                Rm = np.triu(A["R"])
                Rm[np.arange(d), np.arange(d)] = np.abs(np.diagonal(Rm).real) + 1.0
                A["R"] = Rm
            out.append(Case("final_vec", f"final_vec-r{reduced}-b{B}-d{d}", B, m, d, A, state(B), R.params(), reduced))
    return out


GENERIC = dict(init=init_cases, outer_begin=outer_begin_cases, theta=theta_cases, make_y=make_y_cases,
               set_ay=set_ay_cases, grad=grad_cases, gy=gy_cases, prox_in=prox_in_cases, assemble=assemble_cases,
               zasm=zasm_cases, take_z=take_z_cases, make_x=make_x_cases, set_ax=set_ax_cases,
               backtrack=backtrack_cases, iterate=iterate_cases, transpose=transpose_cases, outputs=outputs_cases)


def find(op, tag):
    """The first case of ``op`` whose id contains ``tag``."""
    for c in (GENERIC.get(op) or {"chol": chol_cases, "final_vec": final_vec_cases, "apply_a": apply_a_cases}[op])():
        if tag in c.id:
            return c
    raise KeyError((op, tag))
