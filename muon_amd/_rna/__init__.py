from . import preproc as pp  # noqa: F401
