"""TEST INFRASTRUCTURE -- the final pose solves (LM refit k_pnp_refine, EPnP on the inliers
k_pnp_epnp_s1 / _s3) under structured masks: the catalogue and its helpers.

Expected values are the unchanged CPU restatement's (pyoracle.pnp_refine / pnp_epnp /
pnp_ransac); every comparison with the library is equality of the f64 bit patterns.

LM refit.  Problem: synth.pnp_problem(n, 0.0, seed) (every point consistent, so any mask gives a
meaningful fit); start pose: the true R times a fixed 1e-3 rad rotation, t + (2, -1.5, 3).  The
sizes are the smallest at which each layout of the device reducer exists (lm_blocks / lm_chunk of
rsac_math.h, kLmStage = 4096 staged points, kLmThreads = 512 slots):

  A  n <= 4096            one range, staged once
  B  n = 4097             5 ranges of 820 (the last 817), one block each, staged once
  C  n = 8200             9 ranges of 912 (the last 904); block caps 0 .. 3 (layout(), below)
  D  n = 65537            64 ranges of 1025 = 2 * 512 + 1 (the last 962); caps 0 and 7
  E  n = 262145           64 ranges of 4097 (the last 4034): a range spans two tiles, 4096 + 1;
                          caps 0 and 3

EPnP.  No device entry takes a mask, so the problem is shaped until RANSAC's mask is the wanted
set S: synth.pnp_problem(n, 0.0, 11) with every pixel outside S displaced by 200 - 600 px.

Centre rule (DESIGN.md "Final pose refit"): the refit frame's centre is point 0 when its f32
coordinates are finite, else the lowest masked index.  The check that does not lean on the
restatement (which changes with the code): with mask[0] = 0 and j the lowest masked index, the refit
of the problem whose points3d[0] is non-finite equals the refit of the same problem with
points3d[0] := points3d[j], which takes the finite-point-0 path with the same centre and order.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import pyoracle as O
from rsac import synth

THR, CONF, SEED = 30.0, 0.99, 0x5EED
LM_THREADS, LM_STAGE, LM_ONE_BLOCK, LM_BLOCK_POINTS, LM_MAX_BLOCKS = 512, 4096, 4096, 1024, 64


# ---------------------------------------------------------------------------------------------
# the refit's ranges and the device reducer's layout (rsac_math.h lm_blocks / lm_chunk;
# GpuLmReducer::set_ranges)
# ---------------------------------------------------------------------------------------------
def lm_blocks(n):
    return 1 if n <= LM_ONE_BLOCK else min(-(-n // LM_BLOCK_POINTS), LM_MAX_BLOCKS)


def lm_chunk(n):
    return -(-n // lm_blocks(n))


def ranges(n):
    c = lm_chunk(n)
    return [(r * c, min(n, (r + 1) * c)) for r in range(lm_blocks(n))]


def layout(n, blocks):
    """per block of a launch of `blocks` blocks (block x owns ranges x, x + blocks, ...): (ranges
    owned, index span, "staged once" when the span fits one tile of LM_STAGE else "tile path")"""
    rg = ranges(n)
    out = []
    for x in range(blocks):
        own = rg[x::blocks]
        span = sum(hi - lo for lo, hi in own)
        out.append((len(own), span, "staged once" if span <= LM_STAGE else "tile path"))
    return out


# ---------------------------------------------------------------------------------------------
# problems and start poses
# ---------------------------------------------------------------------------------------------
def _freeze(pr):
    for v in pr.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def problem(n, seed):
    return _freeze(synth.pnp_problem(n, 0.0, seed))


def _small_rotation():
    """Rodrigues of 1e-3 rad about (1, 2, 3) / sqrt(14)"""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = 1e-3
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def start_pose(pr):
    return pr["R"] @ _small_rotation(), pr["t"] + np.array([2.0, -1.5, 3.0])


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---------------------------------------------------------------------------------------------
# the mask catalogue
# ---------------------------------------------------------------------------------------------
def _idx(n, idx):
    m = np.zeros(n, np.uint8)
    m[np.asarray(list(idx), np.int64)] = 1
    return m


def _ones(n):
    return np.ones(n, np.uint8)


def _iid(n):
    return (np.random.default_rng(n).random(n) < 0.5).astype(np.uint8)


def _ranges_only(which):
    def f(n):
        m = np.zeros(n, np.uint8)
        for r, (lo, hi) in enumerate(ranges(n)):
            if which(r):
                m[lo:hi] = 1
        return m
    return f


def _per_range(pick):
    """pick(lo, hi) -> the masked indices of range [lo, hi)"""
    def f(n):
        m = np.zeros(n, np.uint8)
        for lo, hi in ranges(n):
            m[np.asarray(list(pick(lo, hi)), np.int64)] = 1
        return m
    return f


MASKS = {
    "ones": _ones,
    "iid50": _iid,
    "k0": lambda n: _idx(n, []),
    "k1": lambda n: _idx(n, range(300, 301)),
    "k2": lambda n: _idx(n, range(300, 302)),
    "k3": lambda n: _idx(n, range(300, 303)),
    "last7": lambda n: _idx(n, range(n - 7, n)),
    "thread125": lambda n: _idx(n, range(1000, 1008)),  # thread 125's whole bit field (8 indices a thread)
    "mod8is7": lambda n: (np.arange(n) % 8 == 7).astype(np.uint8),
    "lastwave": lambda n: _idx(n, range(3584, 4096)),
    "first512+last": lambda n: _idx(n, list(range(512)) + [n - 1]),
    "range2": _ranges_only(lambda r: r == 2),
    "idx4096": lambda n: _idx(n, [4096]),
    "ranges0and4": _ranges_only(lambda r: r in (0, 4)),
    "oddempty": _ranges_only(lambda r: r % 2 == 0),
    "lastofrange": _per_range(lambda lo, hi: [hi - 1]),
    "first511+lastofrange": _per_range(lambda lo, hi: list(range(lo, lo + 511)) + [hi - 1]),
}

LmCase = namedtuple("LmCase", "group n mask caps")


def _group(group, n, masks, caps=(0,)):
    return [LmCase(group, n, m, tuple(caps)) for m in masks]


LM_CASES = (
    _group("A", 3, ["ones"])
    + _group("A", 600, ["k0", "k1", "k2", "k3"])
    + [c for n in (511, 512, 513, 4095, 4096) for c in _group("A", n, ["ones"])]
    + _group("A", 4096, ["last7", "thread125", "mod8is7", "lastwave", "first512+last"])
    + _group("B", 4097, ["ones", "range2", "idx4096", "ranges0and4"])
    + _group("C", 8200, ["ones", "iid50", "oddempty", "lastofrange"], (0, 1, 2, 3))
    + _group("D", 65537, ["ones", "oddempty"], (0, 7))
    + _group("E", 262145, ["ones", "lastofrange", "first511+lastofrange", "iid50"], (0, 3))
)
LM_IDS = [f"{c.group}-{c.n}-{c.mask}" for c in LM_CASES]
LM_CAPPED = [(c, cap) for c in LM_CASES for cap in c.caps]
LM_CAPPED_IDS = [f"{c.group}-{c.n}-{c.mask}-cap{cap}" for c, cap in LM_CAPPED]


def lm_seed(n):
    return 20 + n % 89


@functools.lru_cache(maxsize=None)
def lm_mask(n, name):
    m = MASKS[name](n)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def lm_inputs(n):
    pr = problem(n, lm_seed(n))
    R0, t0 = start_pose(pr)
    return pr, O.soa_pnp(pr["points3d"], pr["points2d"]), O.cam_from_K(pr["K"]), R0, t0


@functools.lru_cache(maxsize=None)
def lm_expected(n, name):
    """the restatement's refit of case (n, mask name) -> (R, t), computed once"""
    _, soa, cam, R0, t0 = lm_inputs(n)
    R, t, _ = O.pnp_refine(soa, lm_mask(n, name), cam, R0, t0)
    R.setflags(write=False)
    t.setflags(write=False)
    return R, t


# ---------------------------------------------------------------------------------------------
# EPnP on the inliers: problems whose RANSAC mask is the wanted set
# ---------------------------------------------------------------------------------------------
EpCase = namedtuple("EpCase", "n name iters inliers")
EP_SETS = {
    "upper256": lambda n: np.arange(n) >= 256,
    "lower256": lambda n: np.arange(n) < 256,
    "mod512upper": lambda n: np.arange(n) % 512 >= 256,
    "last64": lambda n: np.arange(n) >= 448,
    "tail44": lambda n: np.arange(n) >= 256,
    "100to200+512": lambda n: ((np.arange(n) >= 100) & (np.arange(n) < 200)) | (np.arange(n) == 512),
    "all": lambda n: np.ones(n, bool),
    "from1": lambda n: np.arange(n) >= 1,
}
EP_CASES = [
    EpCase(512, "upper256", 5000, 256),
    EpCase(512, "lower256", 5000, 256),
    EpCase(1024, "mod512upper", 5000, 512),
    EpCase(512, "last64", 30000, 64),
    EpCase(300, "tail44", 30000, 44),
    EpCase(513, "100to200+512", 30000, 101),
    EpCase(256, "all", 2000, 256),
    EpCase(257, "from1", 2000, 256),
]
EP_IDS = [f"{c.n}-{c.name}" for c in EP_CASES]
EP_SEED = 11
EP_BATCH = (3, 4, 5)  # the cases one pnp_ransac_batched call holds (one iteration bound: 30000)


def shaped_problem(n, S, seed=EP_SEED):
    """synth.pnp_problem(n, 0.0, seed) with the pixels outside S moved by 200 - 600 px in a random
    direction -> (points3d, points2d, K)"""
    pr = problem(n, seed)
    rng = np.random.default_rng(seed + 1000)
    out = np.flatnonzero(~np.asarray(S, bool))
    r = rng.uniform(200.0, 600.0, size=len(out))
    th = rng.uniform(0.0, 2.0 * np.pi, size=len(out))
    px = np.array(pr["points2d"])
    px[out] += np.c_[r * np.cos(th), r * np.sin(th)]
    px.setflags(write=False)
    return pr["points3d"], px, pr["K"]


@functools.lru_cache(maxsize=None)
def ep_case(i):
    """-> dict(p3, px, K, S, soa, cam, ransac (the restatement's RANSAC), Re, te (its EPnP on that
    mask, None without a model), Rl, tl (its LM refit from the EPnP pose))"""
    c = EP_CASES[i]
    S = EP_SETS[c.name](c.n)
    p3, px, K = shaped_problem(c.n, S)
    soa, cam = O.soa_pnp(p3, px), O.cam_from_K(K)
    ref = O.pnp_ransac(p3, px, K, THR, CONF, c.iters, SEED)
    m8 = ref["mask"].astype(np.uint8)
    Re, te = O.pnp_epnp(soa, m8, cam)
    R1, t1 = (Re, te) if Re is not None else (ref["R"], ref["t"])
    Rl, tl, _ = O.pnp_refine(soa, m8, cam, R1, t1)
    return dict(p3=p3, px=px, K=K, S=S, soa=soa, cam=cam, ransac=ref, Re=Re, te=te, R1=R1, t1=t1, Rl=Rl, tl=tl)


# ---------------------------------------------------------------------------------------------
# a non-finite first point
# ---------------------------------------------------------------------------------------------
BAD_FIRST = {"nan-x": (0, np.nan), "inf-z": (2, np.inf)}


def with_first_point(p3, value):
    """a copy of p3 whose row 0 is `value` (a row, or (coordinate, scalar) to poison one coordinate)"""
    q = np.array(p3)
    if isinstance(value, tuple):
        q[0, value[0]] = value[1]
    else:
        q[0] = value
    return q


def centre_pair(n, name, kind):
    """the independent check's two problems for LM case (n, mask name) with mask[0] cleared:
    -> (mask, points3d with a non-finite row 0, points3d with row 0 := row j), j the lowest masked"""
    pr = lm_inputs(n)[0]
    m = np.array(lm_mask(n, name))
    m[0] = 0
    j = int(np.flatnonzero(m)[0])
    assert j > 0
    return m, with_first_point(pr["points3d"], BAD_FIRST[kind]), with_first_point(pr["points3d"], pr["points3d"][j])


E2E_KEY = (600, 0.3, 9)  # synth.pnp_problem: 419 RANSAC inliers, point 0 an outlier once it is non-finite


@functools.lru_cache(maxsize=None)
def e2e_problem(kind="nan-x", key=E2E_KEY):
    """synth.pnp_problem(*key) with point 0 poisoned as BAD_FIRST[kind] says (None: left alone)"""
    pr = synth.pnp_problem(*key[:2], seed=key[2])
    if kind is not None:
        k, v = BAD_FIRST[kind]
        pr["points3d"][0, k] = v
    return _freeze(pr)


def ransac_chain(p3, px, K, iters, refine):
    """the restatement's pnp_ransac followed by its final solve -> (ransac dict, R, t)"""
    ref = O.pnp_ransac(p3, px, K, THR, CONF, iters, SEED)
    if ref["best"] < 0:
        return ref, None, None
    soa, cam = O.soa_pnp(p3, px), O.cam_from_K(K)
    m8 = ref["mask"].astype(np.uint8)
    R, t = ref["R"], ref["t"]
    if refine in ("epnp", "epnp+lm"):
        Re, te = O.pnp_epnp(soa, m8, cam)
        if Re is not None:
            R, t = Re, te
    if refine in (True, "lm", "epnp+lm"):
        R, t, _ = O.pnp_refine(soa, m8, cam, R, t)
    return ref, R, t
