"""numpy model of the backward's wave-wide segmented scan (dm2_dpp.h: seg_steps, seg_scan64_n / seg_scan64, run_last_lane) and
of phase D's emit rule (dm2_backward_fast.hip), step for step as the kernel forms them: the six step words from the one ballot
``cont``, four row_shr steps inside the 16-lane rows, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3.

Two forms, as in the kernel: ``fast`` multiplies the shifted value by a 0/1 mask (v_fmac_f32_dpp; finite values only),
``select`` adds and then keeps the sum only where the step is taken."""
import numpy as np

M64 = (1 << 64) - 1
ROW_FIRST = 0x0001000100010001


def cont_word(keys):
    """bit l: lane l > 0 has the key of lane l - 1 (the ballot phase D takes)."""
    c = 0
    for l in range(1, 64):
        if keys[l] == keys[l - 1]:
            c |= 1 << l
    return c


def seg_steps(cont):
    """-> dict(b1, b2, b4, b8, b15, b31), the words of dm2_dpp.h seg_steps, with its operations."""
    b1 = cont & ~ROW_FIRST & M64
    b2 = b1 & (b1 << 1) & M64
    b4 = b2 & (b2 << 2) & M64
    b8 = b4 & (b4 << 4) & M64
    stop = ~cont & M64
    t1, t3, th = (stop >> 16) & 0xFFFF, (stop >> 48) & 0xFFFF, (stop >> 32) & 0xFFFFFFFF
    below = lambda t: ((t & (-t & 0xFFFFFFFF)) - 1) & 0xFFFFFFFF         # the lanes below the lowest set bit; all where none
    r1, r3 = below(t1) & 0xFFFF, below(t3) & 0xFFFF
    return dict(b1=b1, b2=b2, b4=b4, b8=b8, b15=(r1 << 16) | (r3 << 48), b31=below(th) << 32)


def _bits(word):
    return np.array([(word >> l) & 1 for l in range(64)], dtype=bool)


def _shifted(v, K):
    """row_shr:K with bound_ctrl: lane l reads lane l - K of its row, 0 from outside the row."""
    out = np.zeros_like(v)
    for l in range(64):
        if (l & 15) >= K:
            out[l] = v[l - K]
    return out


def _bcast(v, src_of_row):
    """row_bcast: the lanes of the rows in ``src_of_row`` read one lane; the other rows do not execute (their step word is 0)."""
    out = np.zeros_like(v)
    for row, src in src_of_row.items():
        out[16 * row:16 * row + 16] = v[src]
    return out


def seg_scan64(values, cont, form="fast"):
    """Inclusive segmented sum over the runs of ``cont`` -> what every lane holds behind the six steps."""
    k = seg_steps(cont)
    v = np.array(values, dtype=np.float64)
    reads = [(lambda x: _shifted(x, 1), k["b1"]), (lambda x: _shifted(x, 2), k["b2"]), (lambda x: _shifted(x, 4), k["b4"]),
             (lambda x: _shifted(x, 8), k["b8"]), (lambda x: _bcast(x, {1: 15, 3: 47}), k["b15"]),
             (lambda x: _bcast(x, {2: 31, 3: 31}), k["b31"])]
    with np.errstate(invalid="ignore"):
        for read, word in reads:
            take = _bits(word)
            if form == "fast":
                v = v + read(v) * take.astype(np.float64)
            else:
                v = np.where(take, v + read(v), v)
    return v


def emits(keys, active, cont=None):
    """Phase D's emit lanes: the run's last lane (lane l + 1 does not continue l), a key >= 0, an active lane in the run."""
    cont = cont_word(keys) if cont is None else cont
    nact = seg_scan64(np.asarray(active, dtype=np.float64), cont)
    last = ~_bits(cont >> 1)
    return last & (np.asarray(keys) >= 0) & (nact > 0)


def crossing_faces(pairs, wave):
    """The chunk scan's (jx_lo, jx_hi) of thread wave ``wave`` from the kept faces' pair counts: the face with pairs on both
    sides of pair lane 64 wave, and of 64 wave + 64 (-1: none).  Phase D adds for these two and stores for every other face."""
    end = np.cumsum(pairs)
    first = end - np.asarray(pairs)
    lo = 64 * wave
    xl = [j for j in range(len(pairs)) if first[j] < lo < end[j]]
    xh = [j for j in range(len(pairs)) if first[j] < lo + 64 < end[j]]
    return (xl[0] if xl else -1), (xh[0] if xh else -1)


def runs(keys):
    """Maximal stretches of equal neighbouring keys -> [(first lane, last lane)]."""
    out, s = [], 0
    for l in range(1, 65):
        if l == 64 or keys[l] != keys[l - 1]:
            out.append((s, l - 1))
            s = l
    return out
