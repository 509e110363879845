"""Host restatement of the video patch dropout subset draw (valor_amd/csrc/patchdrop.hip valor_patch_keep), in numpy on
tests/dropout_ref.py's Philox4x32-10:
    frame f belongs to draw group g = f // group; patch p of the group has the key w0 | w1 << 32 of
    philox4x32_10(seed, offset + g * Pn + p) (offset: the full 64-bit sum of the by-value offset and the device-resident base);
    the group keeps its k smallest keys, ties to the lower p.
idx [N, k]: the kept positions ascending; slot [N, Pn]: the slot of a kept position, -1 for a dropped one."""
import numpy as np

import dropout_ref as R


def patch_keep_host(seed, offset, N, Pn, k, group=1):
    assert N % group == 0 and 1 <= k <= Pn
    G = N // group
    # counters wrap modulo 2^64 like the kernel's uint64 arithmetic
    ctr = [(int(offset) + g * Pn + p) & R.M64 for g in range(G) for p in range(Pn)]
    w0, w1, _, _ = R.philox4x32_10(int(seed), np.array(ctr, dtype=np.uint64))
    keys = (w0 | (w1 << np.uint64(32))).reshape(G, Pn)
    idx = np.empty((N, k), dtype=np.int32)
    slot = np.full((N, Pn), -1, dtype=np.int32)
    for g in range(G):
        order = np.argsort(keys[g], kind="stable")            # stable: equal keys stay in position order = ties to the lower p
        kept = np.sort(order[:k]).astype(np.int32)
        for f in range(g * group, (g + 1) * group):
            idx[f] = kept
            slot[f, kept] = np.arange(k, dtype=np.int32)
    return idx, slot
