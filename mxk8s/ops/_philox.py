"""Philox4x32-10 (Salmon et al., SC'11) on the host, vectorised with numpy: the
generator of the stochastic MXFP4 quantisers' reference and of their seed
source (``mxfp4.py``); ``native/kernels/mx_philox.h`` is the same function for
the kernels.  Counter-based and stateless: a (counter, key) pair always gives
the same four words."""
from __future__ import annotations

import numpy as np

MUL0, MUL1 = 0xD2511F53, 0xCD9E8D57
WEYL0, WEYL1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key) -> np.ndarray:
    """``counter``: four and ``key``: two integers or integer arrays with values
    in [0, 2^32), broadcast against each other -> ``uint32 [..., 4]``.  The
    32 x 32 -> 64 products are taken in ``uint64``, where they cannot overflow."""
    c = [np.asarray(v, dtype=np.uint64) for v in counter]
    k = [np.asarray(v, dtype=np.uint64) for v in key]
    if len(c) != 4 or len(k) != 2:
        raise ValueError("counter has 4 words and key 2")
    if any((v > _M32).any() for v in c + k):
        raise ValueError("counter and key words must be below 2^32")
    c0, c1, c2, c3 = np.broadcast_arrays(*c, *k)[:4]
    k0, k1 = k
    for _ in range(10):
        p0 = np.uint64(MUL0) * c0
        p1 = np.uint64(MUL1) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(WEYL0)) & _M32
        k1 = (k1 + np.uint64(WEYL1)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)
