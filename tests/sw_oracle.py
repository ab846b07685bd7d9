"""Reference for the shallow-water kernels: one model step in plain torch.

Three functions, one per kernel family of ``csrc/shallow_water.hip``, each
written from the scheme of ``ShallowWater._step_eager`` (same operations in
the same order, so a float64 run of ``step`` equals the eager path bitwise):

``pre``       h, u, v                        -> fe, fn, q, ke
``update``    fe, fn, q, ke, h, u, v, d*_old -> dnh, dnu, dnv, h1, u1, v1
``friction``  u1, v1                         -> u2, v2

They act on a GLOBAL domain of interior ``NY x NX`` (arrays ``(NY + 2,
NX + 2)``) and take every parameter explicitly; nothing here imports the
model.  ``step`` chains the three and returns every intermediate array.

Magnitude companion.  Every function evaluates its expression tree in one
of two arithmetics: ``VALUE`` (the real one) and ``MAGNITUDE``, in which
every input and parameter is replaced by its absolute value, every
subtraction by an addition and every negation by the identity.  ``step``
returns, beside every array ``x``, the array ``mag_x`` obtained by running
the whole step in ``MAGNITUDE`` arithmetic on ``|inputs|``.  ``mag_x`` is
the natural scale of the rounding error of ``x``: a floating-point
evaluation whose longest leaf-to-root path holds ``n`` roundings errs by at
most ``gamma(n) * mag_x`` (Higham, Accuracy and Stability of Numerical
Algorithms, ch. 3), cancellation included.  The GPU tests state their
bounds relative to it.

Decomposition.  ``cut`` slices a global array into the local arrays of a
``P x Q`` process grid (halos are the neighbours' data by construction:
the kernels' "fresh halos" precondition), ``tile_flags`` gives the flag
vector ``ShallowWater._fused_flags`` would produce for that rank,
``tile_cor_base`` its Coriolis base, and ``exchange`` is the model's halo
exchange expressed with tensor indexing only.
"""

from collections import namedtuple

import torch

GRAVITY = 9.81

Params = namedtuple(
    "Params", "dx dy dt nu cor0 cor_dj ab_a ab_b periodic_x")

_I = slice(1, -1)      # interior
_L = slice(None, -2)   # shifted left/down
_R = slice(2, None)    # shifted right/up


def rounded(p, dtype):
    """``p`` with every real parameter rounded to ``dtype`` (what a kernel
    of that dtype holds after the launcher's cast)."""
    def r(x):
        return float(torch.tensor(x, dtype=torch.float64).to(dtype))
    return Params(*[r(x) for x in p[:8]], p.periodic_x)


class _Arith:
    def __init__(self, magnitude):
        self.magnitude = magnitude

    def sub(self, a, b):
        return a + b if self.magnitude else a - b

    def neg(self, a):
        return a if self.magnitude else -a

    def params(self, p):
        if not self.magnitude:
            return p
        return Params(*[abs(x) for x in p[:8]], p.periodic_x)


VALUE = _Arith(False)
MAGNITUDE = _Arith(True)


def _eb(a, kind, periodic_x):
    """Halo refresh of a global array plus the physical walls (the model's
    ``enforce_boundaries`` at world size 1).  Returns a new tensor."""
    a = a.clone()
    if periodic_x:
        a[:, 0] = a[:, -2]
        a[:, -1] = a[:, 1]
    if kind == "u" and not periodic_x:
        a[:, -2] = 0.0
    if kind == "v":
        a[-2, :] = 0.0
    return a


def coriolis(p, ny, dtype):
    """Column ``(ny, 1)`` of ``cor0 + j * cor_dj`` for global rows j."""
    j = torch.arange(ny, dtype=dtype)
    return (p.cor0 + j * p.cor_dj)[:, None]


def pre(h, u, v, p, ar=VALUE):
    """Mass fluxes, potential vorticity and kinetic energy, with the
    halo values the eager path leaves (zeros at closed halos)."""
    p = ar.params(p)
    dx, dy, px = p.dx, p.dy, p.periodic_x
    hc = h.clone()
    hc[0, :] = hc[1, :]
    hc[-1, :] = hc[-2, :]
    hc[:, 0] = hc[:, 1]
    hc[:, -1] = hc[:, -2]
    hc = _eb(hc, "h", px)

    fe = torch.zeros_like(u)
    fn = torch.zeros_like(u)
    fe[_I, _I] = 0.5 * (hc[_I, _I] + hc[_I, _R]) * u[_I, _I]
    fn[_I, _I] = 0.5 * (hc[_I, _I] + hc[_R, _I]) * v[_I, _I]
    fe = _eb(fe, "u", px)
    fn = _eb(fn, "v", px)

    cor = coriolis(p, h.shape[0], h.dtype)
    q = torch.zeros_like(u)
    q[_I, _I] = cor[_I] + ar.sub(
        ar.sub(v[_I, _R], v[_I, _I]) / dx, ar.sub(u[_R, _I], u[_I, _I]) / dy
    )
    q[_I, _I] *= 1.0 / (
        0.25 * (hc[_I, _I] + hc[_I, _R] + hc[_R, _I] + hc[_R, _R])
    )
    q = _eb(q, "h", px)

    ke = torch.zeros_like(u)
    ke[_I, _I] = 0.5 * (
        0.5 * (u[_I, _I] ** 2 + u[_I, _L] ** 2)
        + 0.5 * (v[_I, _I] ** 2 + v[_L, _I] ** 2)
    )
    ke = _eb(ke, "h", px)
    return fe, fn, q, ke


def update(fe, fn, q, ke, h, u, v, dh, du, dv, p, ar=VALUE):
    """Tendencies and the time update ``x + dt * (ab_a * dn + ab_b * do)``
    (``(ab_a, ab_b) = (1, 0)`` is the model's Euler first step), halos
    refreshed and walls applied."""
    p = ar.params(p)
    dx, dy, px = p.dx, p.dy, p.periodic_x
    sub, neg = ar.sub, ar.neg
    dnh = torch.zeros_like(h)
    dnu = torch.zeros_like(h)
    dnv = torch.zeros_like(h)
    dnh[_I, _I] = sub(
        neg(sub(fe[_I, _I], fe[_I, _L])) / dx,
        sub(fn[_I, _I], fn[_L, _I]) / dy,
    )
    dnu[_I, _I] = (
        neg(GRAVITY * sub(h[_I, _R], h[_I, _I])) / dx
        + 0.5 * (
            q[_I, _I] * 0.5 * (fn[_I, _I] + fn[_I, _R])
            + q[_L, _I] * 0.5 * (fn[_L, _I] + fn[_L, _R])
        )
    )
    dnv[_I, _I] = sub(
        neg(GRAVITY * sub(h[_R, _I], h[_I, _I])) / dy,
        0.5 * (
            q[_I, _I] * 0.5 * (fe[_I, _I] + fe[_R, _I])
            + q[_I, _L] * 0.5 * (fe[_I, _L] + fe[_R, _L])
        ),
    )
    dnu[_I, _I] = sub(dnu[_I, _I], sub(ke[_I, _R], ke[_I, _I]) / dx)
    dnv[_I, _I] = sub(dnv[_I, _I], sub(ke[_R, _I], ke[_I, _I]) / dy)

    h1, u1, v1 = h.clone(), u.clone(), v.clone()
    u1[_I, _I] += p.dt * (p.ab_a * dnu[_I, _I] + p.ab_b * du[_I, _I])
    v1[_I, _I] += p.dt * (p.ab_a * dnv[_I, _I] + p.ab_b * dv[_I, _I])
    h1[_I, _I] += p.dt * (p.ab_a * dnh[_I, _I] + p.ab_b * dh[_I, _I])
    return (dnh, dnu, dnv,
            _eb(h1, "h", px), _eb(u1, "u", px), _eb(v1, "v", px))


def _friction_one(w, p, ar):
    dx, dy, px = p.dx, p.dy, p.periodic_x
    gu = torch.zeros_like(w)
    gv = torch.zeros_like(w)
    gu[_I, _I] = p.nu * ar.sub(w[_I, _R], w[_I, _I]) / dx
    gv[_I, _I] = p.nu * ar.sub(w[_R, _I], w[_I, _I]) / dy
    gu = _eb(gu, "u", px)
    gv = _eb(gv, "v", px)
    out = w.clone()
    out[_I, _I] += p.dt * (ar.sub(gu[_I, _I], gu[_I, _L]) / dx
                           + ar.sub(gv[_I, _I], gv[_L, _I]) / dy)
    return out


def friction(u1, v1, p, ar=VALUE):
    """Lateral friction of the post-update velocities, halos refreshed."""
    p = ar.params(p)
    return (_eb(_friction_one(u1, p, ar), "u", p.periodic_x),
            _eb(_friction_one(v1, p, ar), "v", p.periodic_x))


_NAMES = "fe fn q ke dnh dnu dnv h1 u1 v1 u2 v2".split()


def _chain(h, u, v, dh, du, dv, p, ar):
    fe, fn, q, ke = pre(h, u, v, p, ar)
    dnh, dnu, dnv, h1, u1, v1 = update(fe, fn, q, ke, h, u, v, dh, du, dv,
                                       p, ar)
    u2, v2 = friction(u1, v1, p, ar)
    return dict(zip(_NAMES, (fe, fn, q, ke, dnh, dnu, dnv, h1, u1, v1,
                             u2, v2)))


def step(h, u, v, dh, du, dv, p):
    """One model step of the global domain.  Returns a dict with every
    array of ``_NAMES`` and, under ``mag_<name>``, its magnitude
    companion."""
    out = _chain(h, u, v, dh, du, dv, p, VALUE)
    absin = [x.abs() for x in (h, u, v, dh, du, dv)]
    for k, x in _chain(*absin, p, MAGNITUDE).items():
        out["mag_" + k] = x
    return out


# ------------------------------------------------------------ test inputs
def rough_state(ny, nx, periodic_x, seed):
    """Rough global state of interior ``ny x nx``: iid uniform h in [1, 3],
    u, v and the old tendencies in [-1, 1], all float32-representable and
    returned as float64.  Periodic x halos are fresh; closed halos hold
    random data like the rest (the kernels must not depend on them beyond
    what the eager path does), except the wall cells noted below."""
    g = torch.Generator().manual_seed(seed)

    def uni(lo, hi):
        x = torch.rand((ny + 2, nx + 2), generator=g, dtype=torch.float32)
        return (lo + (hi - lo) * x).to(torch.float64)

    h = uni(1.0, 3.0)
    rest = [uni(-1.0, 1.0) for _ in range(5)]
    out = [h] + rest
    if periodic_x:
        for a in out[:3]:
            a[:, 0] = a[:, -2]
            a[:, -1] = a[:, 1]
    else:
        # the four closed-halo cells of the wall column and wall row are
        # zero in every model state (enforce_boundaries zeroes the whole
        # column / row) and the kernels pass closed halos through, so
        # they are part of the input contract.  The INTERIOR of the wall
        # column and row stays rough: a missing wall mask must show.
        u, v = out[1], out[2]
        u[0, -2] = u[-1, -2] = 0.0
        v[-2, 0] = v[-2, -1] = 0.0
    return tuple(out)


# ---------------------------------------------------------- decomposition
def cut(g, P, Q):
    """Local arrays ``{(py, px): tensor}`` of a global array (copies)."""
    nyl, nxl = (g.shape[0] - 2) // P, (g.shape[1] - 2) // Q
    assert nyl * P + 2 == g.shape[0] and nxl * Q + 2 == g.shape[1]
    return {
        (py, px): g[py * nyl:py * nyl + nyl + 2,
                    px * nxl:px * nxl + nxl + 2].clone()
        for py in range(P) for px in range(Q)
    }


def tile_flags(P, Q, py, px, periodic_x, x_wrap=None):
    """[south_open, north_open, west_open, east_open, east_wall,
    north_wall, x_wrap] of rank (py, px).  ``x_wrap`` overrides the last
    entry (0 on a Q == 1 periodic grid = the x halos are exchanged like
    remote ones, the model's ``_force_remote_exchange``)."""
    wrap = int(periodic_x and Q == 1) if x_wrap is None else int(x_wrap)
    return [
        int(py > 0),
        int(py < P - 1),
        int(px > 0 or periodic_x),
        int(px < Q - 1 or periodic_x),
        int((not periodic_x) and px == Q - 1),
        int(py == P - 1),
        wrap,
    ]


def tile_cor_base(p, py, nyl):
    return p.cor0 + py * nyl * p.cor_dj


def exchange(tiles, P, Q, periodic_x):
    """In-place halo exchange of ``{(py, px): tensor}``: every open halo
    cell is set from the neighbour's interior edge (full-height columns
    first, then interior rows, then the open corners — the order of the
    model's exchange, so a column carries its owner's closed-row cells),
    the x wrap included; halo cells of a closed edge stay untouched."""
    def nbr(py, px, dy, dx):
        qy, qx = py + dy, px + dx
        if not 0 <= qy < P:
            return None
        if not 0 <= qx < Q:
            if not periodic_x:
                return None
            qx %= Q
        return tiles[(qy, qx)]

    # halo index on this tile, source index on the neighbour, per offset
    dst = {-1: 0, 1: -1}
    src = {-1: -2, 1: 1}
    for (py, px), t in tiles.items():
        for dx in (-1, 1):
            n = nbr(py, px, 0, dx)
            if n is not None:
                t[:, dst[dx]] = n[:, src[dx]].clone()
    for (py, px), t in tiles.items():
        for dy in (-1, 1):
            n = nbr(py, px, dy, 0)
            if n is not None:
                t[dst[dy], 1:-1] = n[src[dy], 1:-1]
    for (py, px), t in tiles.items():
        for dy in (-1, 1):
            for dx in (-1, 1):
                n = nbr(py, px, dy, dx)
                if n is not None:
                    t[dst[dy], dst[dx]] = n[src[dy], src[dx]]
    return tiles


# ------------------------------------------------- the shared test cases
# (tests/test_sw_oracle.py checks the reference on exactly these inputs,
# tests/test_gpu_sw_stages.py runs the kernels on them)
CONFIGS = [(1, 1, True), (1, 1, False), (3, 1, True), (1, 3, True),
           (1, 3, False), (3, 3, True), (3, 3, False)]  # (P, Q, periodic_x)
SHAPES = [(3, 4), (9, 13), (30, 122)]                   # local (nyl, nxl)
AB = [(1.0, 0.0), (1.6, -0.6)]                          # Euler, AB2
# non-dimensional: every term of the step is O(1) in the result
BASE = dict(dx=1.25, dy=0.75, dt=0.0625, nu=0.75, cor0=0.25, cor_dj=0.0625)

_CASES = {}


def case(P, Q, periodic_x, nyl, nxl, ab, dtype):
    """``(params, state, oracle)`` of one configuration: parameters rounded
    to the kernel's ``dtype``, the rough float64 global state (float32-
    representable) and the float64 ``step`` of it.  Cached; treat the
    result as read-only."""
    key = (P, Q, periodic_x, nyl, nxl, ab, dtype)
    if key not in _CASES:
        p = rounded(Params(**BASE, ab_a=ab[0], ab_b=ab[1],
                           periodic_x=periodic_x), dtype)
        seed = 7 + 1000 * P + 100 * Q + 10 * int(periodic_x) + nyl
        state = rough_state(P * nyl, Q * nxl, periodic_x, seed)
        _CASES[key] = (p, state, step(*state, p))
    return _CASES[key]


# Rounding counts n of the longest path per output, float32 vector kernels
# (the derivation is the docstring of tests/test_gpu_sw_stages.py); the
# bound of a comparison is (n + 1) * 2^-24 * mag, the +1 covering the
# second-order terms of gamma(n) and the float64 reference's own error.
N_PRE = dict(fe=2, fn=2, q=11, ke=3)
N_UPDATE2 = dict(dnh=5, dnu=7, dnv=7, h1=10, u1=12, v1=12)   # rounded inputs
N_MERGED = dict(dnh=6, dnu=18, dnv=18, h1=11, u1=23, v1=23)  # from h, u, v
N_FRICTION = dict(u2=11, v2=11)                              # rounded u1, v1
N_WHOLE = dict(dnh=6, dnu=18, dnv=18, h1=11, u2=33, v2=33)   # whole step

UNIT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}


def bound_k(n, dtype):
    """K of ``|got - ref| <= K * u * mag``.  A float64 kernel is compared
    with a float64 reference that carries up to n roundings of its own."""
    return n + 1 if dtype == torch.float32 else 2 * n + 1


def ratio(got, ref, mag, dtype):
    """max of ``|got - ref| / (u * mag)`` over the given cells; a cell of
    zero magnitude must be matched exactly (ratio inf otherwise)."""
    err = (got.to(torch.float64) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err),
                    err / (UNIT[dtype] * mag))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0
