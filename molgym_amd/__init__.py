"""molgym_amd: the PPO policy / value hot path of molgym on HIP kernels for gfx950."""


def set_deterministic(on: bool, covariant: bool = False, data_parallel: bool = False) -> bool:
    """Turn the library's deterministic mode on or off (process-wide; off by default, MG_DETERMINISTIC=1 in the environment
    starts it on) and return the previous value.  On: SchNetAC's backward, PPO mini-batch step, epoch end and `ppo.train` use
    no float atomics, no side stream and one mini-batch stream, so the same inputs give the same bits on every run and however
    the step is issued.  CovariantAC raises while it is on -- unless its own ordered mode is asked for by name:
    `set_deterministic(True, covariant=True)` turns both switches on (MG_COV_ORDERED=1 in the environment starts the second
    one on), and CovariantAC's training forward, backward and PPO step then take the general launch path with ordered sums: no
    fused small-batch kernels, no graph launch, scratch that grows with the edge count.  `set_deterministic(True)` turns the
    second switch off again, `set_deterministic(False)` both.
    `data_parallel=True` turns a third switch on (MG_DP_ORDERED=1 in the environment starts it on; every call without the keyword
    turns it off): `ppo.train` then keeps the gradient of every mini-batch in a row of its own, gathers the rows of all ranks once
    per epoch and adds them up in global mini-batch order on every rank -- equal rollout data, theta, optimizer state and numpy RNG
    state give the same bits at every world size, one rank included.  It needs the first switch (and, for CovariantAC, the
    second); `train` raises otherwise."""
    from . import _lib
    return _lib.set_deterministic(on, covariant, data_parallel)


def is_deterministic() -> bool:
    from . import _lib
    return _lib.is_deterministic()


def is_deterministic_covariant() -> bool:
    """CovariantAC's ordered mode (the second switch of `set_deterministic`)"""
    from . import _lib
    return _lib.is_deterministic_covariant()


def is_deterministic_data_parallel() -> bool:
    """the data-parallel ordered mode of `ppo.train` (the third switch of `set_deterministic`)"""
    from . import _lib
    return _lib.is_deterministic_data_parallel()


def __getattr__(name):
    # device-resident episodes (molgym_amd/episodes.py), loaded on first use like everything that needs the library
    if name in ('DeviceEpisodes', 'Episode', 'sample_molecules'):
        from . import episodes
        return getattr(episodes, name)
    if name in ('DeviceRollout', 'reference_reward'):  # their trajectories recorded on the device (molgym_amd/rollout.py)
        from . import rollout
        return getattr(rollout, name)
    if name == 'PairReward':  # the reward a device rollout pays without leaving the device (molgym_amd/rewards.py)
        from . import rewards
        return rewards.PairReward
    # relaxation under the pair potential on the device and its host mirror (molgym_amd/relax.py)
    if name in ('relax', 'relax_host', 'relax_canvases', 'energy_forces_canvases', 'Relaxed'):
        import importlib
        module = importlib.import_module('.relax', __name__)  # (`relax` is the module from here on: it is callable)
        return module if name == 'relax' else getattr(module, name)
    # rigid superposition on the device and its host mirror: how far a structure moved (molgym_amd/structure.py)
    if name in ('superpose', 'superpose_host', 'superpose_canvases', 'Superposed'):
        from . import structure
        return getattr(structure, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
