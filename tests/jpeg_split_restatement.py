"""The split entropy decoder (csrc/jpeg_sync_core.hpp, csrc/kernels_jpeg_split.hpp) restated in Python over
tests/jpeg_restatement.py: a restart interval of any length is cut into subsequences, every one is decoded from a guess, and
the guesses are repaired until each lane's entry is its predecessor's exit.  Serial and slow; the definition the kernels and
tools/jpeg_split_check.cpp are held to, bit for bit.

    interval     the bytes offsets[i] .. offsets[i + 1] of the span.  Its DATA end at the first FF followed by anything but 00
                 (an FF that is the interval's very last byte reads as FF), else at the interval's end.
    state        (p, q, b, k) at a symbol boundary: p the byte of the interval that holds the next unread bit (never the 00 of
                 an FF 00 pair), q the bits of it already read, b the block within the MCU, k the zigzag index (0: a DC symbol
                 is expected); or END once a symbol would start at or beyond the data's end.
    symbol       exactly jpeg_restatement.walk's: no code counts as symbol 0 behind 16 bits, a DC symbol above 15 as no code,
                 ZRL and runs past 63 end the block (status RUN), bits beyond the data's end are 0.  A symbol that takes bits
                 from beyond the end sets OVERRUN and leaves the state at the end, so that the next one is END.
    subsequence  j of an interval holds its bytes j * sub_bytes .. (j + 1) * sub_bytes (the last one is shorter; an interval
                 of no bytes has one subsequence of none) and owns the symbols whose first bit lies in it; the last one owns
                 everything behind it as well.  Its cold state is (its first byte -- one later where that is a stuffed 00 --,
                 0, 0, 0).  A lane whose entry lies beyond its subsequence decodes nothing and passes the state through.
    walk_split   the serial walk with the true states: interval i has min(dri, MCUs left) * blocks-per-MCU blocks; symbols
                 that start once they have all ended count for nothing; the walk ends at END, with OVERRUN when a block is
                 then incomplete or missing.  Unreached coefficients are 0 and unreached DC differences are 0, so an
                 unreached block's DC is its predecessor's.
    rounds       round 0: every workgroup of `group` consecutive subsequences (of the whole scan, interval after interval)
                 converges on its own, its first lane cold unless it is an interval's first.  Round r: every workgroup
                 converges again from the exit its predecessor had after round r - 1.  rounds_needed is the number of rounds
                 behind round 0 after which every exit is the true one.
"""
import numpy as np

import jpeg_restatement as R

NOCODE, OVERRUN, RUN, UNSYNCED = 1, 2, 4, 8
END = None


def blocks_of_mcu(h):
    """the component of every block of one MCU, in T.81 order"""
    comps, _, _ = R.geometry(h)
    return [c for c, (ch, cv, _, _, _, _) in enumerate(comps) for _ in range(ch * cv)]


class Interval:
    """one restart interval's bytes, prepared: `real` the unstuffed data bytes, `raw_of[u]` the byte of the interval that holds
    unstuffed byte u (raw_of[len(real)] is the data's end), `u_of` the inverse for the bytes that start one"""

    def __init__(self, raw):
        self.raw = raw = bytes(raw)
        real, raw_of, i = bytearray(), [], 0
        while i < len(raw):
            b = raw[i]
            nxt = raw[i + 1] if i + 1 < len(raw) else 0
            if b == 0xFF and nxt != 0:
                break
            real.append(b)
            raw_of.append(i)
            i += 2 if (b == 0xFF and i + 1 < len(raw)) else 1
        self.end = i
        self.real = bytes(real) + bytes(8)
        self.nreal = len(real)
        self.raw_of = raw_of + [i]
        self.u_of = {p: u for u, p in enumerate(self.raw_of)}


class Tables:
    def __init__(self, h):
        self.comp = blocks_of_mcu(h)
        self.sel = []
        for c in range(h["ncomp"]):
            _, td, ta = h["scan"][c]
            self.sel.append((R.codes(*h["tables"].get((0, td), ([0] * 16, []))), R.codes(*h["tables"].get((1, ta), ([0] * 16, [])))))


def _lookup(tab, peek):
    for length in range(1, 17):
        key = (length, peek >> (16 - length))
        if key in tab:
            return tab[key], length
    return None, 16


def symbol(iv, T, state):
    """one symbol from `state` (not END): (the next state, what it did); END when it would start at or beyond the data's end.
    What it did: (bits of status, the block ended, zigzag index written or None, the value mod 2^16)"""
    p, q, b, k = state
    u = iv.u_of.get(p)
    if u is None or u >= iv.nreal:
        return END, None
    w = int.from_bytes(iv.real[u:u + 5], "big")
    dc, ac = T.sel[T.comp[b]]
    peek = (w >> (24 - q)) & 0xFFFF
    st, done, at, val = 0, False, None, 0
    if k == 0:
        s, length = _lookup(dc, peek)
        if s is None or s > 15:
            st, s = NOCODE, 0
        at, k = 0, 1
    else:
        rs, length = _lookup(ac, peek)
        if rs is None:
            st, rs = NOCODE, 0
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r == 15:
                k += 16
                if k > 63:
                    st |= RUN
            else:
                done = True
        else:
            k += r
            if k <= 63:
                at = k
            else:
                st |= RUN
            k += 1
        if k > 63:
            done = True
    if s:
        val = R.extend((w >> (40 - q - length - s)) & ((1 << s) - 1), s)
    t = q + length + s
    if t > 8 * (iv.nreal - u):
        st |= OVERRUN
        p, q = iv.end, 0
    else:
        p, q = iv.raw_of[u + (t >> 3)], t & 7
    if done:
        b, k = (b + 1) % len(T.comp), 0
    return (p, q, b, k), (st, done, at, val)


def subsequences(length, sub_bytes):
    """[(first byte, byte behind the last)] of an interval of `length` bytes: at least one"""
    n = max(1, -(-length // sub_bytes))
    return [(j * sub_bytes, min((j + 1) * sub_bytes, length)) for j in range(n)]


def cold(iv, lo):
    return (lo + 1 if 0 < lo < len(iv.raw) and iv.raw[lo - 1] == 0xFF and iv.raw[lo] == 0 else lo, 0, 0, 0)


def lane(iv, T, hi, last, entry, emit=None):
    """subsequence .. hi from `entry`: (exit state, blocks that ended).  `emit(done-before, what the symbol did)` sees every
    symbol; it returns False once nothing counts any more (the walk goes on: the states do not care)."""
    st, n = entry, 0
    while st is not END and (last or st[0] < hi):
        nxt, did = symbol(iv, T, st)
        if nxt is END:
            if emit is not None:
                emit(None, st)
            st = END
            break
        if emit is not None:
            emit(did, st)
        n += did[1]
        st = nxt
    return st, n


def walk_split(data, h, dri=None):
    """(per component its (bh, bw, 64) int16 coefficient plane, the uint32 status words) of the split decoder"""
    data = bytes(data)
    comps, mx, my = R.geometry(h)
    T = Tables(h)
    nbm = len(T.comp)
    dri = h["dri"] if dri is None else dri
    dri = dri or mx * my
    offs = h["offsets"]
    planes = [np.zeros((bh, bw, 64), np.int16) for (_, _, bw, bh, _, _) in comps]
    status = np.zeros(len(offs) - 1, np.uint32)
    within = []       # per block of the MCU: (component, row, column) within the MCU
    for c, (ch, cv, _, _, _, _) in enumerate(comps):
        within += [(c, by, bx) for by in range(cv) for bx in range(ch)]
    for i in range(len(offs) - 1):
        iv = Interval(data[offs[i]:offs[i + 1]])
        quota = max(0, min(dri, mx * my - i * dri)) * nbm
        box = {"B": 0, "st": 0}
        diffs = {}

        def emit(did, state, i=i):
            if box["B"] >= quota:
                return
            if did is None:                 # END with blocks of the quota incomplete or missing
                box["st"] |= OVERRUN
                return
            st, done, at, val = did
            box["st"] |= st
            mcu = i * dri + box["B"] // nbm
            c, by, bx = within[box["B"] % nbm]
            row, col = divmod(mcu, mx)
            key = (c, row * comps[c][1] + by, col * comps[c][0] + bx)
            if at == 0:
                diffs[box["B"]] = (key, val)
            elif at is not None:
                planes[c][key[1], key[2], R.ZIGZAG[at]] = R._s16(val)
            box["B"] += done
        lane(iv, T, len(iv.raw), True, (0, 0, 0, 0), emit)
        pred = [0] * h["ncomp"]
        for B in range(quota):
            mcu = i * dri + B // nbm
            c, by, bx = within[B % nbm]
            row, col = divmod(mcu, mx)
            if B in diffs:
                pred[c] = (pred[c] + diffs[B][1]) & 0xFFFF
            planes[c][row * comps[c][1] + by, col * comps[c][0] + bx, 0] = R._s16(pred[c])
        status[i] = box["st"]
    return planes, status


def lanes_of(data, h, sub_bytes):
    """every subsequence of the scan in order: (Interval, first byte, byte behind the last, is the interval's last)"""
    offs = h["offsets"]
    out = []
    for i in range(len(offs) - 1):
        iv = Interval(bytes(data[offs[i]:offs[i + 1]]))
        subs = subsequences(len(iv.raw), sub_bytes)
        out += [(iv, lo, hi, j == len(subs) - 1) for j, (lo, hi) in enumerate(subs)]
    return out


def exits(data, h, sub_bytes):
    """per subsequence (the exit state and block count from its cold state, ... from its true entry)"""
    T = Tables(h)
    out, prev = [], None
    for iv, lo, hi, last in lanes_of(data, h, sub_bytes):
        true_in = (0, 0, 0, 0) if lo == 0 else prev
        true_out = lane(iv, T, hi, last, true_in)
        out.append((lane(iv, T, hi, last, cold(iv, lo)), true_out))
        prev = true_out[0]
    return out


def rounds_needed(data, h, sub_bytes, group):
    """the rounds behind round 0 until every exit is the true one (the module docstring)"""
    T = Tables(h)
    L = lanes_of(data, h, sub_bytes)
    n = len(L)
    memo = {}

    def f(g, entry):
        key = (g, entry)
        if key not in memo:
            iv, lo, hi, last = L[g]
            memo[key] = lane(iv, T, hi, last, entry)[0]
        return memo[key]
    ex = [None] * n
    starts = list(range(0, n, group))

    def converge(g0, entry):
        e = entry
        for g in range(g0, min(g0 + group, n)):
            e = f(g, (0, 0, 0, 0) if L[g][1] == 0 else e)
            ex[g] = e
    for g0 in starts:
        converge(g0, cold(L[g0][0], L[g0][1]))
    true = []
    e = None
    for g in range(n):
        e = f(g, (0, 0, 0, 0) if L[g][1] == 0 else e)
        true.append(e)
    rounds = 0
    while ex != true:
        rounds += 1
        assert rounds <= len(starts), "the fix point must be reached after groups - 1 rounds"
        before = list(ex)
        for g0 in starts[1:]:
            converge(g0, before[g0 - 1])
    return rounds
