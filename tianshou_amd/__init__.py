"""tianshou_amd: the MI355X engine behind Tianshou's `Algorithm` API (README.md).

The sub-modules are imported where they are used (`tianshou_amd.integration`, `tianshou_amd.ppo`, ...); the names below resolve
lazily, so importing the package loads neither torch nor the library."""

_LAZY = {"make_hip_gail": "integration", "GAILConfig": "gail", "GAILDiscriminator": "gail",
         "make_hip_icm": "integration", "ICMConfig": "icm", "ICMEngine": "icm",
         "make_hip_icm_cnn": "integration", "ICMCnnEngine": "icm_cnn"}
__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib

        return getattr(importlib.import_module(f"{__name__}.{_LAZY[name]}"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
