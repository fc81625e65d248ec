"""The device's entropy decode (csrc/jpeg_huffman_kernels.h) restated in plain Python, fed by asep_jpeg_scan_prepare: speculate, synchronise
to a fixed point, place, write, DC sums and the energy bound.  The judge is asep_jpeg_entropy_decode (image_io.load_jpeg_coefficients); the
kernels are written to equal this file step by step, the speculative rule included (an invalid code or index skips one bit, a symbol that
would cross the segment's end stops the subsequence).  Rounds are counted as the library counts them: one round is entry[s] = exit[s - 1]
for every subsequence at once (Jacobi), the speculation is round 0, and the round that changes nothing is counted.
Not a test module: imported by the jpeg scan tests."""
import numpy as np

NATURAL = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
           56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
LOOK_BITS = 9
MAX_BLOCK_ENERGY = 4000000
DAMAGED, REFUSED, NOT_CONVERGED = 1, 2, 4


def round_cap(longest):
    """the cap of simultaneous (Jacobi) rounds for `longest` subsequences in the longest segment: longest - 1 carry correctness to the
    last one, one confirms, one is room; the library bounds its launches by the same count (include/asep_hip.h)"""
    return longest + 1


class _Table:
    def __init__(self, t):
        self.look = list(t.look)
        self.maxcode = list(t.maxcode)
        self.valoff = list(t.valoff)
        self.sym = list(t.sym)
        self.nsym = t.nsym

    def decode(self, v):
        """(length, symbol) of the code at the top of the 32 bits v; length 0 = no code"""
        e = self.look[v >> (32 - LOOK_BITS)]
        if e:
            return e >> 8, e & 255
        for k in range(LOOK_BITS + 1, 17):
            code = v >> (32 - k)
            if code <= self.maxcode[k]:
                i = code + self.valoff[k]
                return (k, self.sym[i]) if 0 <= i < self.nsym else (0, 0)
        return 0, 0


class Scan:
    """a prepared scan (image_io.JpegScan) in the form the steps below index"""

    def __init__(self, scan):
        info = scan.info
        self.ncomp, self.hs, self.vs, self.mcus_w = info.ncomp, info.hs, info.vs, info.mcus_w
        self.bpm = 1 if info.ncomp == 1 else info.hs * info.vs + 2
        self.luma = 1 if self.bpm == 1 else self.bpm - 2
        self.blocks_w = list(info.blocks_w)
        self.comp_blocks = [info.blocks_w[c] * info.blocks_h[c] for c in range(info.ncomp)]
        self.plane_off = [64 * sum(self.comp_blocks[:c]) for c in range(info.ncomp)]
        self.restart_interval = info.restart_interval
        self.qt = [np.asarray(scan.qt[info.qt_index[c]], dtype=np.int64) for c in range(info.ncomp)]
        self.tables = [_Table(scan.tables.dc[c]) for c in range(3)] + [_Table(scan.tables.ac[c]) for c in range(3)]
        raw = bytes(scan.scan[:scan.scan_bytes]) + b"\0" * 8              # reads past the buffer give zeros
        self.win = [int.from_bytes(raw[i:i + 5], "big") for i in range(len(raw) - 4)]
        self.segments = [(int(s["byte_offset"]) * 8, (int(s["byte_offset"]) + int(s["byte_length"])) * 8, int(s["first_mcu"]) * self.bpm,
                          int(s["n_mcus"]) * self.bpm) for s in scan.segments]

    def peek(self, pos):
        return (self.win[pos >> 3] >> (8 - (pos & 7))) & 0xffffffff

    def block_offset(self, g):
        """of scan-order block g in the coefficient buffer, in int16"""
        mcu, b = divmod(g, self.bpm)
        my, mx = divmod(mcu, self.mcus_w)
        if b < self.luma:
            v, u = divmod(b, self.hs)
            return self.plane_off[0] + ((my * self.vs + v) * self.blocks_w[0] + mx * self.hs + u) * 64
        c = b - self.luma + 1
        return self.plane_off[c] + (my * self.blocks_w[c] + mx) * 64


def decode(sc, state, sub_end, seg_end, coef=None, g=0, limit=0):
    """jpeg_huff_decode: from state (pos, blk, idx) until pos >= sub_end -> (exit state, completed blocks, error).  coef None: the
    speculative rule; else the write rule, blocks g, g + 1, ... below limit."""
    pos, blk, idx = state
    write = coef is not None
    completed, err = 0, 0
    while pos < sub_end:
        if write and g >= limit:
            break
        comp = 0 if blk < sc.luma else blk - sc.luma + 1
        v = sc.peek(pos)
        length, sym = sc.tables[(0 if idx == 0 else 3) + comp].decode(v)
        valid, done, s, at, nxt = length != 0, False, 0, 0, idx
        if valid:
            if idx == 0:
                s, nxt = sym, 1
                valid = s <= 11
            else:
                run, s = sym >> 4, sym & 15
                if s == 0:
                    if run == 0:
                        done = True
                    elif run == 15:
                        nxt = idx + 16
                        valid = nxt <= 64
                    else:
                        valid = False
                else:
                    at = idx + run
                    valid = at <= 63 and s <= 10
                    nxt = at + 1
        if not valid:
            if write:
                err = DAMAGED
                break
            pos += 1
            continue
        total = length + s
        if total > seg_end - pos:
            if write:
                err = DAMAGED
            break
        if write and s:
            bits = ((v << length) & 0xffffffff) >> (32 - s)
            coef[sc.block_offset(g) + NATURAL[at]] = bits - (1 << s) + 1 if bits < (1 << (s - 1)) else bits
        pos += total
        idx = nxt
        if done or idx >= 64:
            idx = 0
            blk = 0 if blk + 1 == sc.bpm else blk + 1
            completed += 1
            g += 1
    if write and not err:
        if g >= limit:
            if seg_end - pos >= 8:
                err = DAMAGED
        elif sub_end == seg_end:
            err = DAMAGED
    return (pos, blk, idx), completed, err


def entropy_decode(scan, subseq_bits, max_rounds=None):
    """image_io.JpegScan -> (int16 coefficients as asep_jpeg_entropy_decode lays them out, status, rounds, longest segment in subsequences)"""
    sc = Scan(scan)
    subs = []                                                            # (segment, begin, end, head)
    longest = 0
    for si, (b0, b1, _, _) in enumerate(sc.segments):
        n = -(-(b1 - b0) // subseq_bits)
        longest = max(longest, n)
        subs += [(si, b0 + k * subseq_bits, min(b0 + (k + 1) * subseq_bits, b1), k == 0) for k in range(n)]
    n_coef = 64 * sum(sc.comp_blocks)
    coef = np.zeros(n_coef, dtype=np.int64)
    # 1. speculate
    entry = [(b, 0, 0 if head else 1) for (_, b, _, head) in subs]
    res = [decode(sc, entry[s], subs[s][2], sc.segments[subs[s][0]][1]) for s in range(len(subs))]
    # 2. synchronise
    cap = round_cap(longest) if max_rounds is None else min(round_cap(longest), max_rounds)
    rounds, converged = 0, longest == 1
    while not converged and rounds < cap:
        rounds += 1
        new = [entry[s] if subs[s][3] else res[s - 1][0] for s in range(len(subs))]
        changed = [s for s in range(len(subs)) if new[s] != entry[s]]
        for s in changed:
            entry[s] = new[s]
        for s in changed:
            res[s] = decode(sc, entry[s], subs[s][2], sc.segments[subs[s][0]][1])
        converged = not changed
    if not converged:
        return coef.astype(np.int16), NOT_CONVERGED, rounds, longest
    # 3. place
    first, run = [], 0
    for s, (si, _, _, head) in enumerate(subs):
        if head:
            run = sc.segments[si][2]
        first.append(run)
        run += res[s][1]
    # 4. write
    status = 0
    for s, (si, b, e, head) in enumerate(subs):
        _, seg_end, first_block, n_blocks = sc.segments[si]
        limit = first_block + n_blocks
        start = (b, 0, 0) if head else res[s - 1][0]
        status |= decode(sc, start, e, seg_end, coef, min(first[s], limit), limit)[2]
    # 5. DC sums per component and segment in scan order, then the energy bound
    for c in range(sc.ncomp):
        per = sc.luma if c == 0 else 1
        seg_len = sc.restart_interval * per if sc.restart_interval > 0 else sc.comp_blocks[c]
        pred = 0
        for j in range(sc.comp_blocks[c]):
            mcu, i = divmod(j, per)
            off = sc.block_offset(mcu * sc.bpm + (i if c == 0 else sc.luma + c - 1))
            if j % seg_len == 0:
                pred = 0
            pred += int(coef[off])
            if not -2048 <= pred <= 2047:
                status |= DAMAGED
            coef[off] = max(-32768, min(32767, pred))
        plane = coef[sc.plane_off[c]:sc.plane_off[c] + 64 * sc.comp_blocks[c]].reshape(-1, 64)
        if (((plane * sc.qt[c]) ** 2).sum(axis=1) > MAX_BLOCK_ENERGY).any():
            status |= REFUSED
    return coef.astype(np.int16), status, rounds, longest


FLIPS = 300


def flipped_files(path, mode_index, n=FLIPS):
    """the bytes of `path` with one seeded bit of its scan flipped, n times"""
    raw = open(path, "rb").read()
    sos = raw.index(b"\xff\xda")
    first = sos + 2 + int.from_bytes(raw[sos + 2:sos + 4], "big")
    rng = np.random.default_rng(11 + mode_index)
    for _ in range(n):
        at, bit = int(rng.integers(first, len(raw) - 2)), int(rng.integers(0, 8))
        data = bytearray(raw)
        data[at] ^= 1 << bit
        yield bytes(data)
