"""Host statement of the rules `mg_episode_step_rules` adds to those of tests/episode_ref.py (include/molgym_hip.h), in plain
numpy / Python integers, and `RulesEnvX`, the test double of the reference's other three environment classes.

  * ConstrainedMolecularEnvironment (environment.py:143-175): `_is_valid_action` first asks whether the new atom lies inside
    the convex hull of the scaffold atoms (:155-161, before the distance rules of :164), `find_simplex(q) >= 0` on the Delaunay
    triangulation of the hull vertices (:167-171).  Here: the half spaces of `scipy.spatial.ConvexHull(...).equations`, rows
    (outward unit normal, offset); q is inside iff max_k(((nx*qx + ny*qy) + nz*qz) + d) <= hull_tol.  numpy's float64
    operations round once each, so this is the expression the kernel evaluates with contraction off, bit for bit.  The hull is
    FIXED: a placed atom of the scaffold element would join it in the reference (:156-157), so such formulas are out of scope.
  * RefillableMolecularEnvironment (:178-207): ONE `itertools.cycle` serves resets (:206) and refills (:196) alike; `_is_terminal`
    first returns True on a full canvas (:191-192, no refill consumed), then refills an empty bag while the counter is below
    `num_refills` (:194-197); `reset` zeroes the counter (:204).
  * StochasticEnvironment (:210-249): `reset` draws `sample_formula()` until `is_valid_formula` (:234-236).  One try draws a
    size in [min_size, max_size) (:241-244; max_size when the two are equal) and that many symbols with probability
    count / formula_size (:219,245); it is valid iff sum(count * bond_count[z]) is even (:221-228,249).  The reference draws from
    numpy's global generator, which no device can replay; the draws here come from the keyed generator of csrc/sampling.inc
    (tests/draw_ref.py) in integer arithmetic: r = 24 bits keyed (seed, stream id, stream 4, draw try * 256 + k), k = 0 the
    size, k = 1..size the symbols; size = lo + ((r * (hi - lo)) >> 24); symbol = first i with (r * S) >> 24 < cumulative[i].
    The loop is counted: after `max_tries` invalid tries the row stops with ERROR, where the reference would go on for ever."""
import numpy as np

from tests import draw_ref as D
from tests import episode_ref as R

INACTIVE, PLACED, STOP, TOO_CLOSE, SOLO, FULL, BAG_EMPTY, ERROR = range(8)
REFILLED, OUTSIDE = 8, 9
DONE = (STOP, TOO_CLOSE, SOLO, FULL, BAG_EMPTY, OUTSIDE)
ATOM = (PLACED, FULL, BAG_EMPTY, REFILLED)
BOND_COUNT = {1: 1, 5: 3, 6: 4, 7: 3, 8: 2, 9: 1}  # environment.py:221-228
FORMULA_STREAM = 4


# ---- the hull ---------------------------------------------------------------------------------------------------------------
def hull_planes(points):
    """[P][4] float64: outward unit normal and offset of every facet of the convex hull of `points` (n, 3)"""
    from scipy.spatial import ConvexHull
    return np.ascontiguousarray(ConvexHull(np.asarray(points, dtype=np.float64)).equations, dtype=np.float64)


def hull_values(planes, q):
    """the plane values of the points q (..., 3): (..., P), in the kernel's association"""
    planes, q = np.asarray(planes, dtype=np.float64), np.asarray(q, dtype=np.float64)
    qx, qy, qz = q[..., 0:1], q[..., 1:2], q[..., 2:3]
    return ((planes[:, 0] * qx + planes[:, 1] * qy) + planes[:, 2] * qz) + planes[:, 3]


def hull_max(planes, q):
    return np.fmax.reduce(hull_values(planes, q), axis=-1, initial=-np.inf)  # fmax drops a NaN as the kernel's does


def inside_hull(planes, q, hull_tol=0.0):
    return hull_max(planes, q) <= hull_tol


def inside_scaffold_reference(scaffold_positions, q):
    """environment.py:167-171, on many points at once"""
    from scipy.spatial import ConvexHull, Delaunay
    scaffold_positions = np.asarray(scaffold_positions, dtype=np.float64)
    hull = ConvexHull(scaffold_positions, incremental=False)
    return Delaunay(scaffold_positions[hull.vertices]).find_simplex(np.asarray(q, dtype=np.float64)) >= 0


def fibonacci_sphere(n, radius):
    i = np.arange(n) + 0.5
    ct, ph = 1.0 - 2.0 * i / n, np.pi * (1.0 + 5.0**0.5) * i
    st = np.sqrt(1.0 - ct * ct)
    return radius * np.stack([st * np.cos(ph), st * np.sin(ph), ct], axis=1)


# ---- the formula draw -------------------------------------------------------------------------------------------------------
def u24(seed, sample, stream, draw):
    """rng_u24 of csrc/sampling.inc for broadcastable integer arrays: the 24 bits rng_u01 turns into a float, as int64"""
    U = np.uint64
    sample = np.asarray(sample, dtype=np.int64).astype(np.uint32).astype(U)
    stream, draw = np.asarray(stream, dtype=U), np.asarray(draw, dtype=U)
    sample, stream, draw = np.broadcast_arrays(sample, stream, draw)
    key = (sample.ravel() << U(32)) | ((stream.ravel() << U(24)) ^ draw.ravel())
    h = D.splitmix64(U(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ D.splitmix64(key))
    return (h >> U(40)).astype(np.int64).reshape(sample.shape)


def formula_tries(counts, zs, size_min, size_max, seed, samples, t):
    """try `t` of every stream id of `samples` (n,): (bags (n, Z) int64, valid (n,) bool, sizes (n,) int64)"""
    counts, samples = np.asarray(counts, dtype=np.int64), np.asarray(samples, dtype=np.int64).reshape(-1)
    cum, S = np.cumsum(counts), int(counts.sum())
    sizes = np.full(len(samples), int(size_max), dtype=np.int64)
    if size_min < size_max:
        sizes = int(size_min) + ((u24(seed, samples, FORMULA_STREAM, t * 256) * (int(size_max) - int(size_min))) >> 24)
    k = 1 + np.arange(int(sizes.max()))
    v = (u24(seed, samples[:, None], FORMULA_STREAM, t * 256 + k[None, :]) * S) >> 24
    picks = np.argmax(v[:, :, None] < cum[None, None, :], axis=2)  # the first i with v < cum[i]
    used = k[None, :] <= sizes[:, None]
    bags = np.stack([((picks == i) & used).sum(axis=1) for i in range(len(counts))], axis=1).astype(np.int64)
    bonds = np.array([BOND_COUNT.get(int(z), 0) for z in zs], dtype=np.int64)  # (symbols without one have no count)
    return bags, (bags * bonds[None, :]).sum(axis=1) % 2 == 0, sizes


def formula_try(counts, zs, size_min, size_max, seed, sample, t):
    """try `t` of stream id `sample`: (bag (Z,) int64, valid)"""
    bags, valid, _ = formula_tries(counts, zs, size_min, size_max, seed, [sample], t)
    return bags[0], bool(valid[0])


def draw_formula(counts, zs, size_min, size_max, max_tries, seed, sample):
    """the first valid try of at most `max_tries`: its bag, or None"""
    for t in range(int(max_tries)):
        bag, valid = formula_try(counts, zs, size_min, size_max, seed, sample, t)
        if valid:
            return bag
    return None


# ---- the rules --------------------------------------------------------------------------------------------------------------
def decide(zs, canvas_size, charges, pos, bag, element, q, min_atomic_distance, max_solo_distance, planes=None, hull_tol=0.0,
           refills=0, num_refills=0):
    """the status of one drawn atom: the first rule that applies (environment.py:49-79 with :155-164 and :190-201)"""
    n = len(charges)
    if not 0 <= element < len(zs) or not 0 <= n <= canvas_size:
        return ERROR
    z = zs[element]
    if z != 0 and not bag[element] > 0:
        return ERROR
    if z == 0:
        return STOP
    if planes is not None and len(planes) > 0 and not inside_hull(planes, q, hull_tol):
        return OUTSIDE
    s = R.decide(zs, canvas_size, charges, pos, bag, element, q, min_atomic_distance, max_solo_distance)
    if s == BAG_EMPTY and refills < num_refills:
        return REFILLED
    return s


def episode_step_rules(st, zs, actions, newpos, min_atomic_distance, max_solo_distance, compute_pos, num_refills=0, planes=None,
                       hull_tol=0.0, sampler=None):
    """`mg_episode_step_rules` on the arrays of the dict `st` (those of episode_ref.episode_step plus refills, formula_no),
    updated in place like `newpos`; `sampler`: None or dict(counts, size_min, size_max, max_tries, seed, base, stride).
    Returns (status, element)."""
    E, N = st['charges'].shape
    F = st['formulas'].shape[0]
    cols = actions.shape[1]
    status, element = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
    for e in range(E):
        if st['alive'][e] == 0:
            status[e], element[e] = INACTIVE, -1
            continue
        el = int(np.rint(actions[e, 1 if cols == 6 else 2]))
        n = int(st['natoms'][e])
        element[e] = el
        n_in = n if 0 <= n <= N else 0
        if compute_pos:
            newpos[e] = R.new_position(actions[e], st['pos64'][e], n_in)
        q = newpos[e].copy()
        s = ERROR if n != n_in else decide(zs, N, st['charges'][e, :n], st['pos64'][e, :n], st['bags'][e], el, q, min_atomic_distance,
                                           max_solo_distance, planes, hull_tol, int(st['refills'][e]), num_refills)
        fno = int(st['formula_no'][e])
        new_bag = st['formulas'][(fno + 1) % F]
        if s in DONE and sampler is not None:
            new_bag = draw_formula(sampler['counts'], zs, sampler['size_min'], sampler['size_max'], sampler['max_tries'],
                                   sampler['seed'], sampler['base'] + sampler['stride'] * e)
            if new_bag is None:
                s = ERROR  # nothing else of the row is written
        status[e] = s
        if s == ERROR:
            st['alive'][e] = 0
        elif s in (PLACED, REFILLED):
            st['pos64'][e, n], st['pos32'][e, n] = q, q.astype(np.float32)
            st['charges'][e, n] = zs[el]
            st['bags'][e, el] -= 1
            st['natoms'][e] = n + 1
            if s == REFILLED:
                st['bags'][e] = new_bag
                st['formula_no'][e] = fno + 1
                st['refills'][e] += 1
        else:
            st['pos64'][e] = st['start_pos64'][e]
            st['pos32'][e] = st['start_pos64'][e].astype(np.float32)
            st['charges'][e] = st['start_charges'][e]
            st['natoms'][e] = st['start_natoms'][e]
            st['bags'][e] = new_bag
            st['episode_no'][e] += 1
            st['formula_no'][e] = fno + 1
            st['refills'][e] = 0
    return status, element


class RulesEnvX(R.RulesEnv):
    """`episode_ref.RulesEnv` with the three rule sets.  `formulas`: bags per zs entry.  `scaffold_z`: the hull of the start
    atoms of that element.  `sampler`: dict(counts, size_min, size_max, max_tries, base) -- every reset draws the bag with the
    key `self.draw_key = (seed, stream id)`, which the caller sets before the step that ends an episode (the seed of that
    step), and before construction for episode 0."""

    def __init__(self, canvas_size, zs, formulas, min_atomic_distance=0.6, max_solo_distance=2.0, start=(), num_refills=0,
                 scaffold_z=None, hull_tol=0.0, sampler=None, draw_key=None):
        self.num_refills, self.hull_tol, self.sampler, self.draw_key = num_refills, hull_tol, sampler, draw_key
        self.planes = None
        if scaffold_z is not None:
            self.planes = hull_planes([xyz for label, xyz in start if zs[int(label)] == scaffold_z])
        self.formula_no = -1
        super().__init__(canvas_size, zs, formulas, min_atomic_distance, max_solo_distance, start)

    def reset(self):
        self.episode += 1
        self.formula_no += 1
        self.refills = 0
        self.atoms = list(self.start)
        if self.sampler is not None:
            s = self.sampler
            bag = draw_formula(s['counts'], self.zs, s['size_min'], s['size_max'], s['max_tries'], *self.draw_key)
            if bag is None:
                raise RuntimeError('no valid formula')
            self.bag = [int(c) for c in bag]
        else:
            self.bag = list(self.formulas[self.formula_no % len(self.formulas)])
        self.first_formula = self.formula_no
        self.given = list(self.bag)
        return self._obs()

    def step(self, action):
        element, position = action
        q = np.array([float(x) for x in position], dtype=np.float64)
        s = decide(self.zs, self.N, [self.zs[label] for label, _ in self.atoms], np.array([p for _, p in self.atoms]).reshape(-1, 3),
                   self.bag, int(element), q, self.min_atomic_distance, self.max_solo_distance, self.planes, self.hull_tol,
                   self.refills, self.num_refills)
        if s == ERROR:
            raise RuntimeError(f'element {element} is not in the bag {tuple(self.bag)} / canvas is full')
        if s in ATOM:
            self.atoms.append((int(element), tuple(float(x) for x in q)))
            self.bag[int(element)] -= 1
        if s == REFILLED:  # environment.py:194-197
            self.formula_no += 1
            self.refills += 1
            self.bag = list(self.formulas[self.formula_no % len(self.formulas)])
            self.given = [a + b for a, b in zip(self.given, self.bag)]
        return self._obs(), 0.0, s in DONE, {'status': s}
