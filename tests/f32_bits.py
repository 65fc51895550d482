"""What the numpy-f32 restatements of the fused heads share (helper module, no tests): the float32 guard of every operand, and the
two ways their tests compare f32 results with a kernel's -- by distance in units in the last place, and bit for bit."""
import numpy as np

F32 = np.float32


def _f(a):
    """`a` itself, asserted to be float32: numpy's scalar promotion is the easy way to compute in f64 without noticing"""
    assert isinstance(a, (np.ndarray, np.generic)) and a.dtype == np.float32, getattr(a, "dtype", type(a))
    return a


def ulps(a, b):
    """distance of two float32 values in units in the last place (sign-magnitude order; +0 and -0 are 0 apart)"""
    key = lambda v: (lambda i: np.where(i < 0, np.int64(-(2 ** 31)) - i, i))(np.asarray(v, F32).view(np.int32).astype(np.int64))
    return np.abs(key(a) - key(b))


def bit_equal(a, b):
    """the same shape and the same f32 bits: the sign of a zero and the payload of a NaN included"""
    a, b = np.ascontiguousarray(_f(a)), np.ascontiguousarray(_f(b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bit_equal_any_nan(a, b):
    """`bit_equal`, except that a NaN equals a NaN of any sign and payload (numpy's and the device's default NaNs differ)"""
    a, b = _f(np.ascontiguousarray(a)), _f(np.ascontiguousarray(b))
    nan = np.isnan(a)
    return bool(a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and bit_equal(a[~nan], b[~nan]))
