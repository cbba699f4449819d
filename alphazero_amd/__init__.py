"""alphazero_amd -- MI355X-native self-play engine behind the t0m1ab/alphazero plugin surface.

The package needs libaz_amd.so (HIP, gfx950); importing the engine without it raises ImportError.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # the many-games players, importable from the package; loaded on first use (they pull in torch and the HIP library)
    if name in ("BatchedMCTSPlayer", "BatchedAlphaZeroPlayer"):
        from . import players
        return getattr(players, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
