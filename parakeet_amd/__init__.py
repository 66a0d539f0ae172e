_LAZY = {"HiFiGANGenerator": "hifigan", "HiFiGANInference": "hifigan"}


def __getattr__(name):
    # resolved at first use: importing the package itself stays free of torch and of the engine library
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
