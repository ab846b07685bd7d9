"""Every launchable shallow-water stage against the float64 reference.

Each stage of ``csrc/shallow_water.hip`` is driven directly through
``ext.sw_stage`` on rough data (iid h in [1, 3], u, v and old tendencies in
[-1, 1]) with dx != dy and O(1) non-dimensional parameters, for every rank
of the process grids in ``sw_oracle.CONFIGS`` (so all flag combinations,
``south_open``/``north_open`` and the mixed corners included) at the local
shapes ``sw_oracle.SHAPES``, and compared cell by cell with the matching
slice of the global float64 reference (tests/sw_oracle.py).

The bound.  Every comparison is ``|got - ref| <= K * u * mag``: ``u`` is
2^-24 (float32) or 2^-53 (float64), ``mag`` the reference's magnitude
companion at that cell, and ``K = n + 1`` where ``n`` counts the roundings
on the longest leaf-to-root path of the output's expression tree.  (The
+1 covers the second-order terms of gamma(n) and, for float32, the
reference's own error.  A float64 kernel is compared with a float64
reference that carries up to ``n`` roundings itself: ``K = 2n + 1``.)
Counting rules: an add, subtract, multiply, divide or a rounded constant
(``rdx``, ``rdy``, 9.81f, the float32 ``ab_a``/``ab_b``, a cast
``cor_base``) is one rounding; ``v_rcp_f32`` is its documented 1 ulp = 2
half-ulp roundings; multiplying by 0.5 or 0.25 is exact; a contracted FMA
is no worse than the two roundings it replaces; a sum's count is the
larger operand's + 1, a product's is the sum of its operands' + 1.  The
counts below are for the ``rdx`` (vector) form, which is never shorter
than the division form of the scalar kernels.  Inputs h, u, v, do* and
the parameters dx, dy, dt, nu, cor0, cor_dj are exact (the reference gets
them after rounding to the kernel's dtype).

  from h, u, v (stages 1/11, and inside the merged and fused stages):
    fe, fn = 0.5 * (h + h') * u             add 1, mul 2            n = 2
    ke     = 0.5 * (0.5 * (u^2 + u'^2) + 0.5 * (v^2 + v'^2))
             square 1, inner sum 2, outer sum 3                     n = 3
    q      = (cor + ((v' - v) * rdx - (u' - u) * rdy)) * rcp(0.25 * sum h)
             difference 1, * rdx (itself 1) 3, minus 4, + cor (2) 5;
             sum of four h 3, rcp 5; product 5 + 5 + 1              n = 11
  two-pass update (6/16) from fe, fn, q, ke rounded to the dtype (1 each):
    dnh    = -(fe - fe') * rdx - (fn - fn') * rdy
             difference 2, * rdx 4, minus 5                         n = 5
    dnu    = -G * (h' - h) * rdx + 0.5 * (q * 0.5 * (fn + fn') + ...)
             - (ke' - ke) * rdx
             G term: 1, * G (1) 3, * rdx 5; q term: fn sum 2, * q 4,
             sum of two 5; their sum 6; ke term 4; total            n = 7
    x1     = x + dt * (ab_a * dn + ab_b * do)
             ab_a * dn: n(dn) + 2; + ab_b * do: +1; * dt: +1; + x: +1
             h1: 5 + 5 = 10; u1, v1: 7 + 5                          n = 12
  merged update (8/18-23) and the fused steps' update, from h, u, v:
    dnh    fe 2, difference 3, * rdx 5, minus                       n = 6
    dnu    q (11) * fn sum (3) 15, sum of two 16, + G term 17,
           - ke term (ke 3, difference 4, * rdx 6)                  n = 18
    h1     6 + 5 = 11; u1, v1: 18 + 5                               n = 23
  friction (7/17/27-29) from u1, v1 rounded to the dtype (1):
    x2     = x + dt * ((nu * (e - c) * rdx - nu * (c - w) * rdx) * rdx
                       + (same in y))
             difference 2, * nu 3, * rdx 5, minus 6, * rdx 8,
             x + y 9, * dt 10, + x                                  n = 11
  whole step (30/31/34, 32 + 33): the friction of a computed u1 (23):
             24, 25, 27, 28, 30, 31, 32                             n = 33

These numbers were fixed before any kernel ran and are not tuned.  For
orientation: a dropped or swapped O(1) term that is 1% of ``mag`` is a
ratio near 1.7e5.  No cell is excluded from any comparison; the derived
fields are compared on the rectangles an update stage reads (nothing
reads them elsewhere).

Found by these tests: the float64 instantiations of stages 6 and 8 used the
float32 constant 9.81f for gravity (ratios near 1e8 for dnu, dnv, u, v);
the float64 cases of the two update tests are its regression test.

Harness.  The 16 buffers of a launch are carved out of one allocation
with a two-row sentinel guard band before, between and after them; every
buffer the stage must not read is NaN, every output is pre-filled with the
sentinel, and after the launch the guards and every buffer the stage must
not write are compared bitwise with what was uploaded.
"""

import pytest
import torch

import sw_oracle as o

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64

BUFS = "fe fn q ke h u v dnh dnu dnv doh dou dov h2 u2 v2".split()
SENT = -24680.5  # exact in float32; no output of these inputs comes near
DERIVED = ("fe", "fn", "q", "ke")
DN = ("dnh", "dnu", "dnv")
OUT = ("h2", "u2", "v2")
STATE = ("h", "u", "v", "doh", "dou", "dov")
I_ = (slice(1, -1), slice(1, -1))
IDS = dict(ids=str)


def _ext():
    import mpi4jax_amd._rccl_C as ext
    return ext


def _bits(x):
    return x.view(torch.int32 if x.dtype == F32 else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


class Tile:
    """One rank of one configuration: its flags, Coriolis base and the
    slices of the global reference arrays."""

    def __init__(self, cfg, shape, ab, dtype, py, px, x_wrap=None):
        P, Q, periodic = cfg
        nyl, nxl = shape
        self.p, state, self.ref = o.case(P, Q, periodic, nyl, nxl, ab, dtype)
        self.state = dict(zip(STATE, state))
        self.key = (py, px)
        self.dtype = dtype
        self.ny, self.nx = nyl + 2, nxl + 2
        self.sl = (slice(py * nyl, py * nyl + nyl + 2),
                   slice(px * nxl, px * nxl + nxl + 2))
        self.flags = o.tile_flags(P, Q, py, px, periodic, x_wrap)
        self.cor_base = o.tile_cor_base(self.p, py, nyl)

    def ref_(self, name):
        return self.ref[name][self.sl]

    def mag(self, name):
        return self.ref["mag_" + name][self.sl]

    def inputs(self, names=STATE):
        return {k: self.state[k][self.sl] for k in names}


def tiles_of(cfg, shape, ab, dtype, x_wrap=None):
    return [Tile(cfg, shape, ab, dtype, py, px, x_wrap)
            for py in range(cfg[0]) for px in range(cfg[1])]


class Launch:
    """The guarded allocation of one launch.  ``fill`` maps buffer name ->
    float64 CPU array; ``outputs`` are pre-filled with the sentinel;
    everything else is NaN."""

    def __init__(self, tile, fill, outputs):
        ny, nx, dtype = tile.ny, tile.nx, tile.dtype
        self.tile, self.n, self.guard = tile, ny * nx, 2 * nx
        host = torch.full((17 * self.guard + 16 * self.n,), SENT,
                          dtype=dtype)
        self.is_guard = torch.ones(host.numel(), dtype=torch.bool)
        self.off = {}
        for k, name in enumerate(BUFS):
            off = self.guard + k * (self.n + self.guard)
            self.off[name] = off
            self.is_guard[off:off + self.n] = False
            if name in fill:
                host[off:off + self.n] = fill[name].to(dtype).reshape(-1)
            elif name not in outputs:
                host[off:off + self.n] = float("nan")
        self.host = host
        self.dev = host.cuda()

    def view(self, buf, name):
        off = self.off[name]
        return buf[off:off + self.n].view(self.tile.ny, self.tile.nx)

    def upload(self, name, value):
        """Replace one buffer on the device (and in the expected image)."""
        self.view(self.host, name).copy_(value.to(self.tile.dtype))
        self.view(self.dev, name).copy_(self.view(self.host, name))

    def run(self, stage, writes):
        """Launch, fetch everything, check the guards and the buffers the
        stage must not write; returns {name: CPU array}."""
        t = self.tile
        p = t.p
        _ext().sw_stage(stage, [self.view(self.dev, k) for k in BUFS],
                        p.dx, p.dy, p.dt, p.nu, t.cor_base, p.cor_dj,
                        p.ab_a, p.ab_b, t.flags)
        torch.cuda.synchronize()
        back = self.dev.cpu()
        assert _same_bits(back[self.is_guard], self.host[self.is_guard]), (
            f"stage {stage} tile {t.key}: guard band overwritten")
        for name in BUFS:
            if name not in writes:
                assert _same_bits(self.view(back, name),
                                  self.view(self.host, name)), (
                    f"stage {stage} tile {t.key}: wrote {name}")
        # later launches on this allocation start from this image
        self.host = back
        return {name: self.view(back, name) for name in BUFS}


class Report:
    """Worst err / (u * mag) per (stage, dtype, output) of one test case;
    printed before anything is asserted."""

    def __init__(self):
        self.worst, self.fails = {}, []

    def check(self, stage, tile, name, got, ref, mag, n, where=""):
        dtype = tile.dtype
        k = o.bound_k(n, dtype)
        r = o.ratio(got, ref, mag, dtype)
        tag = "f32" if dtype == F32 else "f64"
        key = (stage, tag, name, k)
        self.worst[key] = max(self.worst.get(key, 0.0), r)
        if not r <= k:
            self.fails.append((stage, tag, name, tile.key, tile.flags,
                               where, r, k))

    def require(self, ok, *what):
        if not ok:
            self.fails.append(what)

    def finish(self):
        for (stage, tag, name, k), r in sorted(self.worst.items()):
            print(f"RATIO stage={stage} {tag} {name} ratio={r:.3f} K={k}")
        assert not self.fails, self.fails[:8]


# ---------------------------------------------- the kernels' fast predicates
def fast_bounds(ny, nx, f):
    """SW_FAST_BOUNDS: (jmin, jmax, imin, imax)."""
    return (1 if f[0] else 2,
            ny - 2 if (f[1] and not f[5]) else ny - 3,
            1 if f[2] else 2,
            nx - 1 if (f[3] and not f[4]) else nx - 2)


def fast_count(stage, ny, nx, f):
    """(fast, slow) pack counts of a vector stage's documented predicate:
    SW_FAST_BOUNDS plus the pack terms (4-column stages 11/16/17/18),
    stage19_pair_fast (19-23), stage27_pair's rule (27-29) and
    s30_fast_out (30-34, the pairs whose friction the LDS pass serves)."""
    jmin, jmax, imin, imax = fast_bounds(ny, nx, f)
    width = 4 if stage in (11, 16, 17, 18) else 2
    fast = slow = 0
    for j in range(ny):
        for i0 in range(0, nx, width):
            box = jmin <= j <= jmax and i0 >= imin and i0 + width <= imax
            if stage == 11:  # no row j-1 input is masked; both x edges open
                ok = (1 <= j <= jmax and i0 >= imin and i0 + 4 <= imax
                      and f[2] and f[3])
            elif stage == 16:  # inputs pre-masked: interior and walls only
                ok = (1 <= j <= (ny - 3 if f[5] else ny - 2) and i0 >= 1
                      and i0 + 4 <= (nx - 2 if f[4] else nx - 1))
            elif stage == 17:
                ok = box and i0 + 5 <= nx
            elif stage == 18:
                ok = box
            elif stage in (19, 20, 21, 22, 23):
                ok = box and i0 + 3 < nx
            elif stage in (27, 28, 29):
                ok = box and i0 + 2 < nx
            else:
                ok = (j - 1 >= jmin and j + 1 <= jmax and i0 - 2 >= imin
                      and i0 + 4 <= imax and i0 + 5 < nx)
            fast += ok
            slow += not ok
    return fast, slow


VECTOR_STAGES = (11, 16, 17, 18, 19, 20, 21, 22, 23, 27, 28, 29,
                 30, 31, 32, 34)


@pytest.mark.parametrize("cfg", o.CONFIGS, **IDS)
def test_largest_shape_reaches_fast_and_slow_paths(cfg):
    """The coverage claim, checked on the host: at the largest shape every
    vector stage runs both its mask-free path and its scalar fallback in
    every configuration it is launched on."""
    P, Q, periodic = cfg
    ny, nx = o.SHAPES[-1][0] + 2, o.SHAPES[-1][1] + 2
    for stage in VECTOR_STAGES:
        if stage in (30, 31, 34) and P * Q > 1:
            continue  # world-1 stages
        fast = slow = 0
        for py in range(P):
            for px in range(Q):
                wrap = 0 if stage == 32 else None
                f = o.tile_flags(P, Q, py, px, periodic, wrap)
                a, b = fast_count(stage, ny, nx, f)
                fast, slow = fast + a, slow + b
        if stage == 11 and cfg == (1, 1, False):
            # sw_stage1v's rule needs both x edges open: a closed-x
            # single rank is all fallback by construction
            assert fast == 0 and slow > 0
        else:
            assert fast > 0 and slow > 0, (stage, cfg, fast, slow)
    # and the fused tiling: several 14 x 60 tiles along both axes
    assert -(-ny // 14) >= 3 and -(-nx // 60) >= 3


def test_smallest_shape_reaches_the_short_ring_enumerations():
    ny, nx = o.SHAPES[0][0] + 2, o.SHAPES[0][1] + 2
    assert ny < 8 and nx < 12  # s30_ring_cell's ny < 8 / nx < 12 branches


# ------------------------------------------------------------ a. PRE
# (fe, fn, q, ke) rectangles an update stage reads: rows, columns
RECT = {"fe": (slice(1, None), slice(0, -1)),
        "fn": (slice(0, -1), slice(1, None)),
        "q": (slice(0, -1), slice(0, -1)),
        "ke": (slice(1, None), slice(1, None))}


def _grid(fn):
    fn = pytest.mark.parametrize("shape", o.SHAPES, **IDS)(fn)
    fn = pytest.mark.parametrize("cfg", o.CONFIGS, **IDS)(fn)
    return gpu(fn)


@_grid
def test_pre_stages(cfg, shape):
    rep = Report()
    for stage, dtype in ((1, F32), (1, F64), (11, F32)):
        for t in tiles_of(cfg, shape, o.AB[0], dtype):
            got = Launch(t, t.inputs(("h", "u", "v")), DERIVED).run(
                stage, DERIVED)
            for name in DERIVED:
                r = RECT[name]
                rep.check(stage, t, name, got[name][r], t.ref_(name)[r],
                          t.mag(name)[r], o.N_PRE[name])
    rep.finish()


# ------------------------------------------------- b. / c. UPDATE stages
def _check_update(rep, stage, t, got, counts, inputs):
    for name, ref in zip(DN + OUT, DN + ("h1", "u1", "v1")):
        rep.check(stage, t, name, got[name][I_], t.ref_(ref)[I_],
                  t.mag(ref)[I_], counts[ref])
    halo = torch.ones(t.ny, t.nx, dtype=torch.bool)
    halo[I_] = False
    for name, src in zip(OUT, ("h", "u", "v")):
        rep.require(
            _same_bits(got[name][halo], inputs[src].to(t.dtype)[halo]),
            stage, t.key, name, "halo is not the input passed through")
    sent = torch.full((int(halo.sum()),), SENT, dtype=t.dtype)
    for name in DN:
        rep.require(_same_bits(got[name][halo], sent),
                    stage, t.key, name, "tendency halo written")


def _unread_poisoned(t):
    """The reference's fe, fn, q, ke slices with NaN outside the
    rectangles an update stage may read."""
    out = {}
    for name in DERIVED:
        a = torch.full((t.ny, t.nx), float("nan"), dtype=F64)
        a[RECT[name]] = t.ref_(name)[RECT[name]]
        out[name] = a
    return out


@_grid
def test_two_pass_update_stages(cfg, shape):
    rep = Report()
    for ab in o.AB:
        for stage, dtype in ((6, F32), (6, F64), (16, F32)):
            for t in tiles_of(cfg, shape, ab, dtype):
                inputs = t.inputs()
                got = Launch(t, {**inputs, **_unread_poisoned(t)},
                             DN + OUT).run(stage, DN + OUT)
                _check_update(rep, stage, t, got, o.N_UPDATE2, inputs)
    rep.finish()


@_grid
def test_merged_update_stages(cfg, shape):
    rep = Report()
    for ab in o.AB:
        for stage, dtype in ((8, F32), (8, F64), (18, F32), (19, F32)):
            for t in tiles_of(cfg, shape, ab, dtype):
                inputs = t.inputs()
                got = Launch(t, inputs, DN + OUT).run(stage, DN + OUT)
                _check_update(rep, stage, t, got, o.N_MERGED, inputs)
                if stage != 19:
                    continue
                for twin in (20, 21, 22, 23):  # the same stage19_cells
                    again = Launch(t, inputs, DN + OUT).run(twin, DN + OUT)
                    for name in DN + OUT:
                        rep.require(_same_bits(again[name], got[name]),
                                    twin, t.key, name, "differs from 19")
    rep.finish()


# ------------------------------------------------------- d. FRICTION
@_grid
def test_friction_stages(cfg, shape):
    rep = Report()
    ab = o.AB[1]
    for stage, dtype in ((7, F32), (7, F64), (17, F32), (27, F32)):
        for t in tiles_of(cfg, shape, ab, dtype):
            fill = {"u": t.ref_("u1"), "v": t.ref_("v1")}
            got = Launch(t, fill, ("u2", "v2")).run(stage, ("u2", "v2"))
            halo = torch.ones(t.ny, t.nx, dtype=torch.bool)
            halo[I_] = False
            for name, src in (("u2", "u"), ("v2", "v")):
                rep.check(stage, t, name, got[name][I_], t.ref_(name)[I_],
                          t.mag(name)[I_], o.N_FRICTION[name])
                rep.require(_same_bits(got[name][halo],
                                       fill[src].to(dtype)[halo]),
                            stage, t.key, name, "halo not passed through")
            if stage != 27:
                continue
            # 28 (halo-independent pairs) + 29 (ring pairs) = 27, bitwise
            part = {s: Launch(t, fill, ("u2", "v2")).run(s, ("u2", "v2"))
                    for s in (28, 29)}
            for name in ("u2", "v2"):
                sent = torch.full_like(got[name], SENT)
                w27 = _bits(got[name]) != _bits(sent)
                w28 = _bits(part[28][name]) != _bits(sent)
                w29 = _bits(part[29][name]) != _bits(sent)
                rep.require(bool(w27.all()), 27, t.key, name,
                            "27 left cells unwritten")
                rep.require(not bool((w28 & w29).any()), t.key, name,
                            "28 and 29 overlap")
                rep.require(torch.equal(w28 | w29, w27), t.key, name,
                            "28 + 29 do not cover 27")
                both = torch.where(w28, part[28][name], part[29][name])
                rep.require(_same_bits(both, got[name]), t.key, name,
                            "28/29 values differ from 27")
    rep.finish()


# ----------------------------------------------------- e. WHOLE STEP
WORLD1 = [c for c in o.CONFIGS if c[0] * c[1] == 1]
STEP_OUT = DN + OUT


def _check_dn(rep, stage, t, got):
    halo = torch.ones(t.ny, t.nx, dtype=torch.bool)
    halo[I_] = False
    sent = torch.full((int(halo.sum()),), SENT, dtype=t.dtype)
    for name in DN:
        rep.check(stage, t, name, got[name][I_], t.ref_(name)[I_],
                  t.mag(name)[I_], o.N_WHOLE[name])
        rep.require(_same_bits(got[name][halo], sent),
                    stage, t.key, name, "tendency halo written")


@gpu
@pytest.mark.parametrize("shape", o.SHAPES, **IDS)
@pytest.mark.parametrize("cfg", WORLD1, **IDS)
def test_single_rank_step_stages(cfg, shape):
    """Stages 30, 31 and 34: a complete step, halo ring included."""
    rep = Report()
    for ab in o.AB:
        (t,) = tiles_of(cfg, shape, ab, F32)
        first = None
        for stage in (30, 31, 34):
            # 34 stages u', v' in fe/fn; 30/31 must leave them alone
            writes = STEP_OUT + (("fe", "fn") if stage == 34 else ())
            got = Launch(t, t.inputs(), STEP_OUT).run(stage, writes)
            _check_dn(rep, stage, t, got)
            for name, ref in zip(OUT, ("h1", "u2", "v2")):
                rep.check(stage, t, name, got[name], t.ref_(ref),
                          t.mag(ref), o.N_WHOLE[ref])
            if stage == 30:
                first = got
            elif stage == 31:
                for name in STEP_OUT:
                    rep.require(_same_bits(got[name], first[name]),
                                31, name, "differs from stage 30")
    rep.finish()


@_grid
def test_multi_rank_step_stages(cfg, shape):
    """Stage 32, exchange(fe, fn), stage 33, exchange(h2, u2, v2) on every
    rank of the grid (world 1: with x_wrap = 0, the forced-remote form)."""
    P, Q, periodic = cfg
    rep = Report()
    for ab in o.AB:
        ts = tiles_of(cfg, shape, ab, F32, x_wrap=0)
        runs = {t.key: Launch(t, t.inputs(), STEP_OUT) for t in ts}
        mid = {t.key: runs[t.key].run(32, STEP_OUT + ("fe", "fn"))
               for t in ts}
        for name in ("fe", "fn"):  # the u', v' strip exchange
            strip = o.exchange({k: g[name].clone() for k, g in mid.items()},
                               P, Q, periodic)
            for k, v in strip.items():
                runs[k].upload(name, v)
        end = {t.key: runs[t.key].run(33, OUT) for t in ts}
        final = {name: o.exchange({k: g[name].clone()
                                   for k, g in end.items()}, P, Q, periodic)
                 for name in OUT}
        for t in ts:
            _check_dn(rep, "32+33", t, end[t.key])
            s, n, w, e = t.flags[:4]
            closed = torch.zeros(t.ny, t.nx, dtype=torch.bool)
            if not s:
                closed[0, :] = True
            if not n:
                closed[-1, :] = True
            if not w:
                closed[:, 0] = True
            if not e:
                closed[:, -1] = True
            inputs = t.inputs(("h", "u", "v"))
            for name, ref, src in zip(OUT, ("h1", "u2", "v2"),
                                      ("h", "u", "v")):
                got = final[name][t.key]
                rep.check("32+33", t, name, got[~closed],
                          t.ref_(ref)[~closed], t.mag(ref)[~closed],
                          o.N_WHOLE[ref])
                rep.require(_same_bits(got[closed],
                                       inputs[src].to(F32)[closed]),
                            "32+33", t.key, name, "closed halo changed")
    rep.finish()
