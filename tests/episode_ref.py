"""Host statement of the rules `mg_episode_step` applies (include/molgym_hip.h), in plain numpy / Python floats, and a
`RulesEnv` test double with the step / reset contract of tests/fake_env.py (zero reward).

The rules are the reference environment's without its reward call (environment.py:49-118,134-140): null element -> stop; a
new atom closer than `min_atomic_distance` to an existing one -> too close; an H / F / Cl / Br with no other kind of atom
within `max_solo_distance` on a non-empty canvas -> solo; otherwise the atom is placed and the episode ends when the canvas
is full or the bag is empty.  An element index out of range or absent from the bag is an error, checked first.  Every ending
resets the row to its start canvas and the next formula of its own cycle (episode k uses formulas[k % F]).

The distance is float64, sqrt((dx*dx + dy*dy) + dz*dz): numpy's elementwise float64 operations round once each, so this is
the expression the kernel evaluates with contraction off, bit for bit."""
import numpy as np

INACTIVE, PLACED, STOP, TOO_CLOSE, SOLO, FULL, BAG_EMPTY, ERROR = range(8)
DONE = (STOP, TOO_CLOSE, SOLO, FULL, BAG_EMPTY)
SOLO_ZS = (1, 9, 17, 35)  # H, F, Cl, Br (environment.py:105)


def distances(pos, q):
    """float64 distances of the rows of `pos` (n, 3) from `q` (3,)"""
    pos, q = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(q, dtype=np.float64)
    dx, dy, dz = pos[:, 0] - q[0], pos[:, 1] - q[1], pos[:, 2] - q[2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def new_position(action6, pos, n):
    """where a 6-column float32 action row places its atom (to_action_space, agent.py:147-163): the focused atom's float64
    position plus the float32 product distance * direction; the origin on an empty canvas"""
    a = np.asarray(action6, dtype=np.float32)
    focus = int(np.rint(a[0]))
    if n > 0 and 0 <= focus < n:
        return np.asarray(pos[focus], dtype=np.float64) + (a[2] * a[3:6]).astype(np.float64)
    return np.zeros(3)


def decide(zs, canvas_size, charges, pos, bag, element, q, min_atomic_distance, max_solo_distance):
    """the status of one drawn atom (`element` indexes zs, `q` its float64 position) on a canvas holding the atoms
    `charges` (n,) at `pos` (n, 3) with the bag `bag`: the first rule that applies"""
    n = len(charges)
    if not 0 <= element < len(zs) or not 0 <= n <= canvas_size:
        return ERROR
    z = zs[element]
    if z != 0 and not bag[element] > 0:
        return ERROR
    if z == 0:
        return STOP
    d = distances(pos, q)
    if np.any(d < min_atomic_distance):
        return TOO_CLOSE
    if z in SOLO_ZS and n > 0:
        heavy = np.array([c not in SOLO_ZS for c in charges], dtype=bool)
        if not np.any(d[heavy] < max_solo_distance):
            return SOLO
    if n == canvas_size:
        return ERROR  # a legal atom and no slot for it
    if n + 1 == canvas_size:
        return FULL
    left = sum(bag) - 1
    return BAG_EMPTY if left == 0 else PLACED


def episode_step(st, zs, actions, newpos, min_atomic_distance, max_solo_distance, compute_pos):
    """`mg_episode_step` on the arrays of the dict `st` (pos64, pos32, charges, bags, natoms, alive, episode_no, start_pos64,
    start_charges, start_natoms, formulas), updated in place like `newpos`; returns (status, element)"""
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
            newpos[e] = new_position(actions[e], st['pos64'][e], n_in)
        q = newpos[e].copy()
        s = ERROR if n != n_in else decide(zs, N, st['charges'][e, :n], st['pos64'][e, :n], st['bags'][e], el, q,
                                           min_atomic_distance, max_solo_distance)
        status[e] = s
        if s == ERROR:
            st['alive'][e] = 0
        elif s == PLACED:
            st['pos64'][e, n], st['pos32'][e, n] = q, q.astype(np.float32)
            st['charges'][e, n] = zs[el]
            st['bags'][e, el] -= 1
            st['natoms'][e] = n + 1
        else:
            ep = int(st['episode_no'][e])
            st['pos64'][e] = st['start_pos64'][e]
            st['pos32'][e] = st['start_pos64'][e].astype(np.float32)
            st['charges'][e] = st['start_charges'][e]
            st['natoms'][e] = st['start_natoms'][e]
            st['bags'][e] = st['formulas'][(ep + 1) % F]
            st['episode_no'][e] = ep + 1
    return status, element


def molecule_obeys_rules(zs, canvas_size, numbers, positions, bag, num_start, min_atomic_distance, max_solo_distance):
    """every atom after the first `num_start` of a finished molecule was a legal placement on the atoms before it, out of
    `bag` (counts per zs entry)"""
    bag = list(bag)
    for k in range(num_start, len(numbers)):
        el = zs.index(int(numbers[k]))
        s = decide(zs, canvas_size, list(numbers[:k]), positions[:k], bag, el, positions[k], min_atomic_distance, max_solo_distance)
        if s not in (PLACED, FULL, BAG_EMPTY) or (s != PLACED and k != len(numbers) - 1):
            return False
        bag[el] -= 1
    return True


def collect_episodes(records, zs, num_formulas, start_numbers, start_positions):
    """the finished episodes of a step record, by step and then environment.  `records`: per step a dict of per-environment
    arrays status, element, newpos (E, 3), logp, v; `start_numbers[e]` / `start_positions[e]`: the atoms every episode of
    environment e starts from.  Each episode: dict(env, formula, numbers, positions (n, 3) float64, status, logp, v)."""
    E = len(start_numbers)
    open_ = [dict(numbers=[], positions=[], logp=[], v=[]) for _ in range(E)]
    count, out = [0] * E, []
    for rec in records:
        for e in range(E):
            s = int(rec['status'][e])
            if s in (INACTIVE, ERROR):
                continue
            cur = open_[e]
            cur['logp'].append(float(rec['logp'][e]))
            cur['v'].append(float(rec['v'][e]))
            if s in (PLACED, FULL, BAG_EMPTY):
                cur['numbers'].append(int(zs[int(rec['element'][e])]))
                cur['positions'].append(np.asarray(rec['newpos'][e], dtype=np.float64).copy())
            if s != PLACED:
                numbers = np.array(list(start_numbers[e]) + cur['numbers'], dtype=np.int64)
                positions = np.array(list(np.asarray(start_positions[e], dtype=np.float64).reshape(-1, 3)) + cur['positions'],
                                     dtype=np.float64).reshape(-1, 3)
                out.append(dict(env=e, formula=count[e] % num_formulas, numbers=numbers, positions=positions, status=s,
                                logp=np.array(cur['logp'], dtype=np.float32), v=np.array(cur['v'], dtype=np.float32)))
                count[e] += 1
                open_[e] = dict(numbers=[], positions=[], logp=[], v=[])
    return out


class RulesEnv:
    """an environment with the MolecularEnvironment step / reset contract (tests/fake_env.py) that applies exactly the rules
    above: reward 0.0, `info['status']` the status code; an illegal element raises RuntimeError as the reference does"""

    def __init__(self, canvas_size, zs, formulas, min_atomic_distance=0.6, max_solo_distance=2.0, start=()):
        self.N, self.zs, self.formulas = canvas_size, list(zs), [tuple(int(c) for c in f) for f in formulas]
        self.min_atomic_distance, self.max_solo_distance = min_atomic_distance, max_solo_distance
        self.start = [(int(label), tuple(float(x) for x in xyz)) for label, xyz in start]  # (label, position) canvas items
        self.episode = -1
        self.reset()

    def _obs(self):
        canvas = list(self.atoms) + [(0, (0.0, 0.0, 0.0))] * (self.N - len(self.atoms))
        return tuple(canvas), tuple(self.bag)

    def reset(self):
        self.episode += 1
        self.atoms, self.bag = list(self.start), list(self.formulas[self.episode % len(self.formulas)])
        return self._obs()

    def step(self, action):
        element, position = action
        q = np.array([float(x) for x in position], dtype=np.float64)
        s = decide(self.zs, self.N, [self.zs[label] for label, _ in self.atoms], np.array([p for _, p in self.atoms]).reshape(-1, 3),
                   self.bag, int(element), q, self.min_atomic_distance, self.max_solo_distance)
        if s == ERROR:
            raise RuntimeError(f'element {element} is not in the bag {tuple(self.bag)} / canvas is full')
        if s in (PLACED, FULL, BAG_EMPTY):
            self.atoms.append((int(element), tuple(float(x) for x in q)))
            self.bag[int(element)] -= 1
        return self._obs(), 0.0, s != PLACED, {'status': s}
