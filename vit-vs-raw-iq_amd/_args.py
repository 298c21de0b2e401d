"""Argument checkers, and the one limit (MAX_LENGTH), every generator, receiver, stage and front end shares.  A leaf: nothing
of the package is imported here."""
from __future__ import annotations

import math
import numbers
import operator

_F32_MAX = 3.4028234663852886e38
MAX_LENGTH = 8192            # one workgroup keeps one frame in LDS: len * 8 bytes <= 64 KB


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise TypeError(f"{what} must be a number, got {v!r}")
    v = float(v)
    if not math.isfinite(v) or abs(v) > _F32_MAX:
        raise ValueError(f"{what} must be finite, got {v!r}")
    return v


def _flag(v, what):
    if not isinstance(v, bool) and not (isinstance(v, int) and v in (0, 1)):
        raise TypeError(f"{what} must be True or False, got {v!r}")
    return bool(v)


def _index(v, what, lo=0, hi=None):
    if isinstance(v, bool):
        raise TypeError(f"{what} must be an integer, got {v!r}")
    try:
        i = operator.index(v)
    except TypeError:
        raise TypeError(f"{what} must be an integer, got {v!r}") from None
    if i < lo or (hi is not None and i > hi):
        raise ValueError(f"{what} must be >= {lo}" + (f" and <= {hi}" if hi is not None else "") + f", got {v!r}")
    return i
