def __getattr__(name):
    # resolved on first use: `import lookoncetohear_amd` itself stays free of torch (build.py runs before anything is built)
    if name in ("Resampler", "resample_bank"):
        from . import resample
        return getattr(resample, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
