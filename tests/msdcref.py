"""numpy reference of the MSCB combine step (pn2_msdc_combine / pn2_msdc_combine_bwd, include/pn2.h): channel_shuffle(sum or cat of the MSDC branches, groups)
and the adjoint of the cat mode.  Everything is float32 arithmetic in a fixed order, so the device kernels are compared with it bit for bit; bf16 storage is
modelled as float32 values rounded to nearest even on 16 mantissa-and-exponent bits (helpers below turn them into the 16-bit patterns and back)."""
import numpy as np


def src_index(Cw, groups):
    """src(j) = (j % groups) * (Cw / groups) + j / groups: output channel j of channel_shuffle(., groups) reads input channel src(j)."""
    assert Cw % groups == 0
    j = np.arange(Cw)
    return (j % groups) * (Cw // groups) + j // groups


def bf16_bits(x):
    """float32 array -> uint16 bf16 patterns, round to nearest even (finite inputs; an overflow rounds to infinity as the hardware convert does)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    """uint16 bf16 patterns -> the float32 values they stand for."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


def _store(x, bf16):
    return bf16_round(x) if bf16 else np.asarray(x, dtype=np.float32)


def combine(parts, groups, mode, bf16=False):
    """parts: 1 to 4 float32 arrays [M][Cpart] holding storage-representable values.  mode 'sum': ((p0 + p1) + p2) + p3 in float32, rounded once to the storage
    type (one part: a move); mode 'cat': the concatenation, a move.  The result is read through src_index."""
    assert 1 <= len(parts) <= 4 and mode in ("sum", "cat")
    parts = [np.asarray(p, dtype=np.float32) for p in parts]
    if mode == "cat":
        row = np.concatenate(parts, axis=1)
    elif len(parts) == 1:
        row = parts[0]
    else:
        acc = parts[0]
        with np.errstate(over="ignore", invalid="ignore"):
            for p in parts[1:]:
                acc = (acc + p).astype(np.float32)
        row = _store(acc, bf16)
    return np.ascontiguousarray(row[:, src_index(row.shape[1], groups)])


def combine_bwd(dy, n, groups, prefill=None, accumulate=None, bf16=False):
    """Adjoint of mode 'cat': d_i[p][c] (+)= dy[p][dst(i * Cpart + c)], dst the inverse of src.  prefill[i] / accumulate[i]: what part i holds before the call and
    whether the gradient is added to it (float32 add, rounded once) or replaces it."""
    dy = np.asarray(dy, dtype=np.float32)
    Cw = dy.shape[1]
    assert Cw % n == 0
    g = np.empty_like(dy)
    g[:, src_index(Cw, groups)] = dy                 # y[j] = in[src(j)]  =>  d in[src(j)] = dy[j]
    outs = []
    for i, gi in enumerate(np.split(g, n, axis=1)):
        if accumulate is not None and accumulate[i]:
            with np.errstate(over="ignore", invalid="ignore"):
                gi = _store((np.asarray(prefill[i], dtype=np.float32) + gi).astype(np.float32), bf16)
        outs.append(np.ascontiguousarray(gi))
    return outs
