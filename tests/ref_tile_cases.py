"""Case sets that hold the tile coding against the reference's OWN source (oracle/_ref/ref_tiles, built by oracle/Makefile from the
unmodified base/src/projectors/tile_coding.cpp and its header), shared by tests/test_oracle_ref_tiles.py (CPU: oracle against the
binary), tools/record_ref_envs.py (writes tests/golden/ref_tiles.npz) and tests/test_gpu_ref_tiles.py (GPU: grlx_project against the
fixture).  Fixed seeds, no clock.

A spec is a dict (name, tilings, memory, res, wrap); `wrap` may have another length than `res` (configure refuses that).  The inputs
of a spec are at most MAX_ROWS rows, each tagged with what it is there for (TAGS).  A claim sequence is a list of operations on one
small claim table: single projections (claim), variant projections (claim under safe = 2 only) and one reset.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import configs
from tests import oracle_binding as ob

REF_BIN = os.path.join(ob.ORACLE_DIR, "_ref", "ref_tiles")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")                   # oracle/Makefile's default
REF_SOURCES = [os.path.join(REFERENCE, "base", "src", "projectors", "tile_coding.cpp"),
               os.path.join(REFERENCE, "base", "include", "grl", "projectors", "tile_coding.h")]
FIXTURE = os.path.join(ob.ROOT, "tests", "golden", "ref_tiles.npz")

MAX_ROWS = 256
MAX_DIMS = 8                                                                 # GRLX_MAX_DIMS, ORC_MAX_DIMS
BOUND = 2.0 ** 30                                                            # |x * scaling| below it: what grlx_project and the queries admit
HASH_MEMORY = 4099          # the table the full hash sums are read from (tile_hash): createHashSum does not depend on the memory

TAGS = ["uniform", "negative", "zero", "tile_edge", "tile_edge_below", "tile_edge_above", "wrap", "bound"]
TAG = {t: i for i, t in enumerate(TAGS)}


def reference_sources_present():
    return all(os.path.exists(p) for p in REF_SOURCES)


# ------------------------------------------------------------------------------------------------------ specs ---
def _of(name, ts):
    return dict(name=name, tilings=ts.tilings, memory=ts.memory, res=[ts.resolution[i] for i in range(ts.dims)],
                wrap=[ts.wrapping[i] for i in range(ts.dims)])


def specs():
    """every projector of tests/configs.py, the five of tests/test_gpu_parity.py::_tile_specs, and the shapes neither has"""
    out = []
    for name, make in (("pendulum", configs.pendulum), ("acrobot", configs.acrobot), ("cart_pole_ac", configs.cart_pole_ac),
                       ("pendulum_ac", configs.pendulum_ac), ("walker", configs.compass_walker), ("pendulum_qv", configs.pendulum_qv),
                       ("acrobot_qv", configs.acrobot_qv), ("cart_pole_q", configs.cart_pole_q)):
        spec = make(None, 1)[1]
        out.append(_of(name + "/critic", spec.projector))
        if spec.actor_projector.dims > 0 and spec.agent in (ob.AGENT_AC, ob.AGENT_QV):
            out.append(_of(name + "/actor", spec.actor_projector))
    seen, unique = set(), []
    for s in out:                                                         # the same projector under two names is held once
        key = (s["tilings"], s["memory"], tuple(s["res"]), tuple(s["wrap"]))
        if key not in seen:
            seen.add(key); unique.append(s)
    out = unique
    for i, (T, mem, res, wrap) in enumerate([
            (16, 8388608, [0.31415, 3.1415, 3], [6.283, 0, 0]), (16, 8388608, [2.5, 0.157075, 2.5, 1.57075], [0, 6.283, 0, 0]),
            (8, 1000003, [0.5, 0.25], [0, 0]), (32, 4096, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [0, 0, 1.2, 0, 0, 0]), (1, 65536, [1.0], [0])]):
        s = dict(name=f"parity{i}", tilings=T, memory=mem, res=res, wrap=wrap)
        key = (T, mem, tuple(float(r) for r in res), tuple(float(w) for w in wrap))
        if key not in seen:
            seen.add(key); out.append(s)
    out += [
        dict(name="dims8_wrap_last", tilings=16, memory=1048576, res=[0.5, 0.25, 1.0, 2.0, 0.125, 0.3, 0.7, 0.5], wrap=[0, 0, 0, 0, 0, 0, 0, 2.0]),
        dict(name="dims8_tilings32", tilings=32, memory=1000003, res=[0.5, 0.25, 1.0, 2.0, 0.125, 0.3, 0.7, 0.5], wrap=[0] * 8),
        dict(name="wrap_several", tilings=16, memory=999983, res=[0.5, 1.0, 0.25, 2.0, 0.5], wrap=[4.0, 0, 1.0, 0, 3.0]),
        dict(name="tilings1_wrap", tilings=1, memory=257, res=[0.5, 2.0], wrap=[0, 6.0]),
        dict(name="wrap_rounds", tilings=16, memory=65536, res=[1.0, 1.0], wrap=[(4 + 0.0009) / 16, 0]),     # 0.0009 from an integer: accepted, rounded
    ]
    return out


def refused_specs():
    """what TileCodingProjector::configure throws on: scaled wrapping more than 0.001 from an integer, a wrapping vector of another length"""
    return [dict(name="wrap_not_integer", tilings=16, memory=65536, res=[1.0, 1.0], wrap=[(4 + 0.002) / 16, 0]),
            dict(name="wrap_not_integer_last", tilings=16, memory=8388608, res=[2.5, 0.157075, 2.5, 2.5], wrap=[0, 0, 0, 6.283]),
            dict(name="wrap_wrong_length", tilings=16, memory=65536, res=[0.5, 0.25, 1.0], wrap=[0, 2.0])]


def tile_spec(s, cls=None):
    """the spec as an oracle (or, with cls, a grlx) structure; None where the fixed arrays cannot say it (another wrapping length)"""
    if len(s["wrap"]) != len(s["res"]):
        return None
    ts = (cls or ob.TileSpec)()
    ts.tilings, ts.memory, ts.dims = s["tilings"], s["memory"], len(s["res"])
    for i, (r, w) in enumerate(zip(s["res"], s["wrap"])):
        ts.resolution[i] = r; ts.wrapping[i] = w
    return ts


# ----------------------------------------------------------------------------------------------------- inputs ---
def _inside(x, scaling, sign):
    """the double nearest to x, towards 0, whose product with the scaling is below 2^30 in magnitude"""
    x = sign * abs(x)
    while not abs(x * scaling) < BOUND:
        x = np.nextafter(x, 0.0)
    return float(x)


def inputs(s, seed):
    T, res, wrap = s["tilings"], np.array(s["res"], np.float64), np.array(s["wrap"], np.float64)
    D = len(res)
    scaling = T / res
    step = res / T                                                        # the width of a tile in a single tiling's offset grid
    rng = np.random.default_rng(seed)
    rows, tags = [], []

    def add(tag, x):
        rows.append(np.array(x, np.float64)); tags.append(TAG[tag])

    for _ in range(16):
        add("uniform", rng.uniform(-40, 40, D))
    for _ in range(8):
        add("negative", rng.uniform(-40, 0, D))
    for v in (0.0, -1e-12, 5e-324, -5e-324):
        add("zero", np.full(D, v))
    # multiples of resolution / tilings and their two neighbours: every dimension at once, then one dimension among uniform others
    for j in range(6):
        k = rng.integers(-600, 600, D)
        at = k * step
        add("tile_edge", at); add("tile_edge_below", np.nextafter(at, -np.inf)); add("tile_edge_above", np.nextafter(at, np.inf))
    for i in range(D):
        base = rng.uniform(-40, 40, D)
        at, below, above = base.copy(), base.copy(), base.copy()
        for k in rng.integers(-600, 600, 64):                             # a multiple one of whose neighbours quantises to the next tile
            v = int(k) * step[i]
            lo, hi = np.nextafter(v, -np.inf), np.nextafter(v, np.inf)
            if len({np.floor(lo * scaling[i]), np.floor(v * scaling[i]), np.floor(hi * scaling[i])}) > 1:
                break
        at[i], below[i], above[i] = v, lo, hi
        add("tile_edge", at); add("tile_edge_below", below); add("tile_edge_above", above)
    # both sides of the wrap and of its multiples, several turns either way
    for i in np.nonzero(wrap)[0]:
        w = wrap[i]
        for v in (w, np.nextafter(w, 0), w - 0.5 * step[i], w + 0.5 * step[i], -0.5 * step[i], -w, np.nextafter(-w, -np.inf), 7 * w + 0.3 * step[i], -5 * w - 0.3 * step[i]):
            x = rng.uniform(-40, 40, D); x[i] = v
            add("wrap", x)
    # x * scaling within 2 of +-2^30, inside the bound: the last quantised coordinates the int cast holds
    for j, d in enumerate((1.75, 1.25, 0.5, 0.0)):
        for sign in (1.0, -1.0):
            i = (2 * j + (sign < 0)) % D
            x = rng.uniform(-40, 40, D); x[i] = _inside((BOUND - d) / scaling[i], scaling[i], sign)
            add("bound", x)
    cases = dict(x=np.array(rows), tag=np.array(tags, np.int32))
    assert len(tags) <= MAX_ROWS
    _check_coverage(s, cases)
    return cases


def _check_coverage(s, cases):
    """the properties the rows are there for, from the inputs alone"""
    T, res, wrap = s["tilings"], np.array(s["res"], np.float64), np.array(s["wrap"], np.float64)
    D = len(res)
    scaling = T / res
    x, tag = cases["x"], cases["tag"]
    q = x * scaling
    assert np.isfinite(x).all() and (np.abs(q) < BOUND).all(), "every row is inside what grlx_project admits"
    at, below, above = (x[tag == TAG[t]] * scaling for t in ("tile_edge", "tile_edge_below", "tile_edge_above"))
    assert len(at) == len(below) == len(above) == 6 + D
    assert (np.abs(at[:6] - np.round(at[:6])) < 1e-9).all(), "the products land on or beside an integer"
    crossed = (np.floor(below) != np.floor(at)) | (np.floor(above) != np.floor(at))
    assert crossed[:6].any(axis=1).all() and all(crossed[6 + i, i] for i in range(D)), "a neighbour quantises to the neighbouring tile"
    assert (x[tag == TAG["negative"]] < 0).all() and (x[tag == TAG["zero"]] == 0).any() and (x[tag == TAG["zero"]] < 0).any()
    for i in np.nonzero(wrap)[0]:
        w = round(wrap[i] * scaling[i])
        qi = np.floor(q[tag == TAG["wrap"], i])
        assert (qi >= w).any() and ((qi < w) & (qi >= 0)).any() and (qi < 0).any() and (qi <= -w).any() and (qi >= 2 * w).any()
    b = np.abs(q[tag == TAG["bound"]])
    assert ((b >= BOUND - 2) & (b < BOUND)).any(axis=1).all() and (q[tag == TAG["bound"]] < 0).any() and (b.max() > BOUND - 1e-6)


def beyond_bound(s):
    """[(x row, dimension)]: the first value outside the bound on either side, NaN and the infinities, each in one dimension of an
    otherwise plain row -- what grlx_project refuses"""
    res = np.array(s["res"], np.float64)
    scaling = s["tilings"] / res
    out = []
    for j, (kind, sign) in enumerate((("first", 1.0), ("first", -1.0), ("nan", 1.0), ("inf", 1.0), ("inf", -1.0))):
        i = j % len(res)
        x = np.linspace(-1.0, 1.0, len(res))
        if kind == "first":
            x[i] = np.nextafter(_inside(BOUND / scaling[i], scaling[i], sign), sign * np.inf)
            assert not abs(x[i] * scaling[i]) < BOUND
        else:
            x[i] = np.nan if kind == "nan" else sign * np.inf
        out.append((x, i))
    return out


# ---------------------------------------------------------------------------------------------- the reference ---
def hexes(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=np.float64).ravel())


def ask(lines, binary=REF_BIN, errors=False):
    out = subprocess.run([binary], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines), f"{binary}: {len(out)} answers to {len(lines)} commands"
    if not errors:
        for line, answer in zip(lines, out):
            assert not answer.startswith("error"), f"{line.split()[0]}: {answer}"
    return [answer.split() for answer in out]


def configure_line(s, memory=None, safe=0):
    return f"tile_configure {s['tilings']} {memory or s['memory']} {safe} {len(s['res'])} {hexes(s['res'])} {hexes(s['wrap'])}".rstrip()


def reference_indices(s, x, binary=REF_BIN):
    """project(in) of every row: [n, tilings] uint32"""
    answers = ask([configure_line(s)] + [f"tile_project {hexes(r)}" for r in x], binary)[1:]
    return np.array([[int(w) for w in a] for a in answers], np.uint32).reshape(len(x), s["tilings"])


def reference_hashes(s, x, binary=REF_BIN):
    """the full hash sums of every row, read out of the claim table of a HASH_MEMORY-slot projector of the same shape"""
    answers = ask([configure_line(s, memory=HASH_MEMORY, safe=1)] + [f"tile_hash {hexes(r)}" for r in x], binary)[1:]
    return np.array([[int(w) for w in a] for a in answers], np.uint32).reshape(len(x), s["tilings"])


def reference_refuses(s, binary=REF_BIN):
    return ask([configure_line(s)], binary, errors=True)[0][0] == "error"


# ------------------------------------------------------------------------------------------------- the oracle ---
def oracle_indices(s, x, full_hash=False):
    L = ob.load()
    ts = tile_spec(s)
    out = np.zeros((len(x), ts.tilings), np.uint32)
    tmp = (C.c_uint32 * ts.tilings)()
    for i, r in enumerate(x):
        rc = (L.orc_tile_project_hash if full_hash else L.orc_tile_project)(C.byref(ts), (C.c_double * ts.dims)(*r), tmp)
        assert rc == 0
        out[i] = tmp[:]
    return out


def oracle_refuses(s):
    ts = tile_spec(s)
    tmp = (C.c_uint32 * 32)()
    return ob.load().orc_tile_project(C.byref(ts), (C.c_double * ts.dims)(), tmp) != 0


# -------------------------------------------------------------------------------------------- claim sequences ---
SINGLE, VARIANTS, RESET = 0, 1, 2
CLAIM_MEMORIES = (61, 64, 257)
CLAIM_VARIANTS = (-3.0, 0.0, 3.0)
CLAIM_SPEC = dict(name="claims", tilings=4, res=[0.31415, 3.1415, 3.0], wrap=[6.283, 0, 0])
CLAIM_OPS = 300
MAX_OCCUPANCY = 0.75        # the reference's walk does not end on a full table


class ClaimTable:
    """the oracle's claim function over a table this object holds"""

    def __init__(self, s, memory, safe):
        self.L = ob.load()
        self.ts = tile_spec(dict(s, memory=memory))
        self.memory, self.safe, self.T = memory, safe, s["tilings"]
        self.table = (C.c_int32 * memory)(*([-1] * memory))

    def reset(self):
        for i in range(self.memory):
            self.table[i] = -1

    def project(self, x, claim):
        """-> (slot indices [T], home slots h % memory [T])"""
        h = (C.c_uint32 * self.T)()
        assert self.L.orc_tile_project_hash(C.byref(self.ts), (C.c_double * self.ts.dims)(*x), h) == 0
        home = [v % self.memory for v in h]
        out = (C.c_uint32 * self.T)()
        self.L.orc_tile_claim(self.table, self.memory, h, self.T, int(claim), out)
        return list(out), home

    def single(self, x):
        return self.project(x, True)

    def variants(self, base):
        idx, home = [], []
        for v in CLAIM_VARIANTS:
            i, h = self.project(list(base) + [v], self.safe > 1)
            idx += i; home += h
        return idx, home

    def claims(self):
        return np.array(self.table[:], np.int32)

    def occupancy(self):
        return float((self.claims() != -1).sum()) / self.memory


def claim_sequence(memory, safe):
    """CLAIM_OPS operations: kind [n], x [n, 3] (a variant projection reads its base from the first two).  New inputs come while the
    table has room; past that the sequence returns to inputs it has seen, so that occupancy stays at or below MAX_OCCUPANCY.  The
    first of a fixed series of seeds whose sequence crowds the table and walks past its end, both onto slot 0 and beyond it."""
    for attempt in range(200):
        seq, wrapped, longest, peak = _claim_sequence(memory, safe, attempt)
        if min(wrapped) > 0 and longest >= 2 and peak > 0.5:
            return seq
    raise AssertionError("no sequence whose probing walk goes past the table's end")


def _claim_sequence(memory, safe, attempt):
    rng = np.random.default_rng(1000 * memory + safe + 100000 * attempt)
    s = CLAIM_SPEC
    table = ClaimTable(s, memory, safe)
    kinds, xs, seen = [], [], {SINGLE: [], VARIANTS: []}
    wrapped, longest = [0, 0], 0                                          # walks that ended on slot 0 / beyond it, after the table's end
    peak = 0.0
    for n in range(CLAIM_OPS):
        if n == CLAIM_OPS // 2:
            kinds.append(RESET); xs.append(np.zeros(3)); table.reset(); seen = {SINGLE: [], VARIANTS: []}
            continue
        kind = VARIANTS if rng.random() < 0.4 else SINGLE
        fresh = np.array([rng.uniform(-7, 7), rng.uniform(-12, 12), CLAIM_VARIANTS[rng.integers(3)]])
        room = (table.claims() != -1).sum() + s["tilings"] * (len(CLAIM_VARIANTS) if kind == VARIANTS else 1) <= MAX_OCCUPANCY * memory
        if not room and not seen[kind]:
            kind = SINGLE if kind == VARIANTS else VARIANTS
        x = fresh if room else seen[kind][rng.integers(len(seen[kind]))]  # an input seen in the same kind of projection claims nothing new
        idx, home = table.single(x) if kind == SINGLE else table.variants(x[:2])
        wrapped[0] += sum(i == 0 and h > 0 for i, h in zip(idx, home))
        wrapped[1] += sum(0 < i < h for i, h in zip(idx, home))
        longest = max([longest] + [(i - h) % memory for i, h in zip(idx, home)])
        peak = max(peak, table.occupancy())
        assert table.occupancy() <= MAX_OCCUPANCY, "the sequence would fill the table"
        kinds.append(kind); xs.append(x); seen[kind].append(x)
    return dict(kind=np.array(kinds, np.int32), x=np.array(xs), memory=memory, safe=safe), wrapped, longest, peak


def claim_lines(seq):
    s = dict(CLAIM_SPEC, memory=seq["memory"])
    lines = [configure_line(s, safe=seq["safe"])]
    for kind, x in zip(seq["kind"], seq["x"]):
        if kind == RESET:
            lines += ["tile_claims", "tile_reset"]
        elif kind == SINGLE:
            lines.append(f"tile_project {hexes(x)}")
        else:
            lines.append(f"tile_project_variants {hexes(x[:2])} {len(CLAIM_VARIANTS)} {hexes(CLAIM_VARIANTS)}")
    return lines + ["tile_claims"]


def reference_claims(seq, binary=REF_BIN):
    """-> [per operation: the indices returned (a reset: the claim table before it)], the final claim table"""
    answers = ask(claim_lines(seq), binary)[1:]
    out, at = [], 0
    for kind in seq["kind"]:
        out.append([int(w) for w in answers[at]])
        at += 2 if kind == RESET else 1
    return out, [int(w) for w in answers[at]]


def oracle_claims(seq):
    table = ClaimTable(CLAIM_SPEC, seq["memory"], seq["safe"])
    out = []
    for kind, x in zip(seq["kind"], seq["x"]):
        if kind == RESET:
            out.append(table.claims().tolist()); table.reset()
        else:
            out.append((table.single(x) if kind == SINGLE else table.variants(x[:2]))[0])
    return out, table.claims().tolist()
