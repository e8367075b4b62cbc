"""molgym_amd: the PPO policy / value hot path of molgym on HIP kernels for gfx950."""


def set_deterministic(on: bool) -> bool:
    """Turn the library's deterministic mode on or off (process-wide; off by default, MG_DETERMINISTIC=1 in the environment
    starts it on) and return the previous value.  On: SchNetAC's backward, PPO mini-batch step, epoch end and `ppo.train` use
    no float atomics, no side stream and one mini-batch stream, so the same inputs give the same bits on every run and however
    the step is issued.  CovariantAC raises while it is on."""
    from . import _lib
    return _lib.set_deterministic(on)


def is_deterministic() -> bool:
    from . import _lib
    return _lib.is_deterministic()
