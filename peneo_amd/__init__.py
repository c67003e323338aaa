"""peneo_amd — MI355X-native forward/backward hot path of PEneo."""
__version__ = "0.1.0"


# Deterministic mode: bit-reproducible training steps.  Thin forwards to peneo_amd.hip, imported on use so that
# `import peneo_amd` stays free of torch and of the shared library.
def set_deterministic(flag_or_mode) -> None:
    """False / 0 off, True / 1 on, 2 strict (order-dependent calls raise).  Process-wide."""
    from . import hip
    hip.set_deterministic(flag_or_mode)


def is_deterministic() -> bool:
    from . import hip
    return hip.is_deterministic()


def deterministic(mode=2):
    """Context manager: ``with peneo_amd.deterministic(): step()`` - restores the mode it found."""
    from . import hip
    return hip.deterministic(mode)
