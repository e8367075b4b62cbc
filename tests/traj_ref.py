"""Host statement of the trajectory store of `DeviceRollout` (include/molgym_hip.h: mg_traj_record, mg_traj_status,
mg_episode_cut, mg_traj_gae) in numpy / Python floats.

Environment e's step t of a T-step collect is sample e * T + t.  The rule rewards: STOP pays 0.0, TOO_CLOSE / SOLO / OUTSIDE
`min_reward`, an atom-placing status the caller's reward; a reward below `min_reward` becomes `min_reward` and ends the episode
(status LOW_REWARD unless the step had ended it already).  The segmented GAE walks every environment's slots backwards in
float64, one operation at a time in `k_gae`'s order -- delta = (rew + gamma * next_v) - val, adv = delta + (gamma * lam) * adv,
ret = rew + gamma * ret -- which is also the order of `DynamicPPOBuffer.finish_path`."""
import numpy as np

INACTIVE, PLACED, STOP, TOO_CLOSE, SOLO, FULL, BAG_EMPTY, ERROR, REFILLED, OUTSIDE, LOW_REWARD = range(11)
ENDS = (STOP, TOO_CLOSE, SOLO, FULL, BAG_EMPTY, OUTSIDE, LOW_REWARD)
ATOM = (PLACED, FULL, BAG_EMPTY, REFILLED)


def rule_reward(status, min_reward):
    """what mg_traj_status writes: the reward the rules alone decide (0.0 where the caller's reward goes)"""
    return float(min_reward) if status in (TOO_CLOSE, SOLO, OUTSIDE) else 0.0


def pay(status, reward, min_reward):
    """(status, reward) of an atom-placing step once the caller's reward is known (environment.py:66-70)"""
    if reward < min_reward:
        return (LOW_REWARD if status in (PLACED, REFILLED) else status), float(min_reward)
    return status, float(reward)


class TrajStore:
    """the arrays of the store for E environments and T steps, filled row by row as the kernels fill them"""

    def __init__(self, E, T, N, Z, cols):
        S = E * T
        self.E, self.T = E, T
        self.pos64, self.pos = np.zeros((S, N, 3), np.float64), np.zeros((S, N, 3), np.float32)
        self.charges, self.bags = np.zeros((S, N), np.int32), np.zeros((S, Z), np.float32)
        self.actions = np.zeros((S, cols), np.float32)
        self.logp, self.val, self.rew = np.zeros(S, np.float64), np.zeros(S, np.float64), np.zeros(S, np.float64)
        self.status = np.zeros(S, np.int32)

    def record(self, t, pos64, charges, bags, actions, logp32, v32, alive=None):
        """mg_traj_record: the canvases (E, N, 3) / (E, N), bags (E, Z), action rows and float32 logp / v of step t"""
        for e in range(self.E):
            if alive is not None and not alive[e]:
                continue
            s = e * self.T + t
            self.pos64[s], self.pos[s] = pos64[e], np.asarray(pos64[e], np.float64).astype(np.float32)
            self.charges[s], self.bags[s], self.actions[s] = charges[e], bags[e], actions[e]
            self.logp[s], self.val[s] = float(np.float32(logp32[e])), float(np.float32(v32[e]))

    def set_status(self, t, status, min_reward):
        """mg_traj_status"""
        for e in range(self.E):
            if status[e] == INACTIVE:
                continue
            s = e * self.T + t
            self.status[s], self.rew[s] = status[e], rule_reward(int(status[e]), min_reward)

    def set_rewards(self, t, rows, rewards, min_reward):
        """the caller's rewards of the atom rows of step t, and the cut of those below min_reward; returns the rows whose open
        episode was cut"""
        cut = []
        for e, r in zip(rows, rewards):
            s = e * self.T + t
            before = int(self.status[s])
            self.status[s], self.rew[s] = pay(before, float(r), min_reward)
            if self.status[s] == LOW_REWARD:
                cut.append(int(e))
        return cut


def segmented_gae(status, rew, val, last_val, gamma, lam):
    """mg_traj_gae on (E, T) arrays: (adv, ret (E, T) float64, num_done (E,), len_sum (E,), len_sq (E,))"""
    status = np.asarray(status)
    E, T = status.shape
    rew, val = np.asarray(rew, np.float64).reshape(E, T), np.asarray(val, np.float64).reshape(E, T)
    adv, ret = np.zeros((E, T)), np.zeros((E, T))
    num_done, len_sum, len_sq = np.zeros(E, np.int64), np.zeros(E), np.zeros(E)
    gl = float(gamma) * float(lam)
    for e in range(E):
        next_v, acc_a, acc_r = float(last_val[e]), 0.0, float(last_val[e])
        end = -1
        for t in range(T - 1, -1, -1):
            if int(status[e, t]) in ENDS:
                if end >= 0:
                    n = end - t
                    num_done[e] += 1
                    len_sum[e] += n
                    len_sq[e] += n * n
                end, next_v, acc_a, acc_r = t, 0.0, 0.0, 0.0
            r, v = float(rew[e, t]), float(val[e, t])
            delta = (r + gamma * next_v) - v
            acc_a = delta + gl * acc_a
            acc_r = r + gamma * acc_r
            adv[e, t], ret[e, t], next_v = acc_a, acc_r, v
        if end >= 0:
            n = end + 1
            num_done[e] += 1
            len_sum[e] += n
            len_sq[e] += n * n
    return adv, ret, num_done, len_sum, len_sq


def normalize(adv):
    """buffer.py:104-110: population standardisation, no epsilon"""
    adv = np.asarray(adv, np.float64)
    return (adv - np.mean(adv)) / np.std(adv)
