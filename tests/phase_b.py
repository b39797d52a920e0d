"""TEST INFRASTRUCTURE ONLY -- Phase B of the reference's parallel encoder,
restated serially in Python, macroblock by macroblock, with the topNz /
leftNz / topNzDC / leftNzDC state exactly as the Go code keeps it.  It stays
serial on purpose: that is what makes it an independent check of the kernels'
parallel context derivation (webp_amd/csrc/tokens.hip).

  collect_coeff_stats / collect_level_stats   internal/lossy/encode_proba.go:10-113
  collect_all_stats                           encode_proba.go:171-313 (= collectMBStats,
                                              encode_parallel.go:1602-1707, per MB)
  optimize_proba / branch_cost                encode_proba.go:117-168
  record_coeffs / record_level                internal/lossy/encode_token.go:115-300
  record_mb_tokens                            internal/lossy/encode_frame.go:647-759
  record_all_tokens                           encode_proba.go:317-353 (rerecordAllTokens)
  skip_proba                                  encode_parallel.go:1595-1597

Tables come from oracle/vp8_tables.h (tests/test_tables.py pins that file to
the Go source), as tests/encode_quality.py reads its own.  Also here: a
generator of synthetic, self-consistent wg_mb_enc records.
"""
import os
import re

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(name):
    txt = open(os.path.join(_ROOT, "oracle", "vp8_tables.h")).read()
    body = txt[txt.index(name + "["):]
    body = body[body.index("{") + 1:body.index("};")]
    return [int(x) for x in re.findall(r"-?\d+", body)]


BANDS = _table("vp8_bands")
ZIGZAG = _table("vp8_zigzag")
PROBA0 = np.array(_table("vp8_coeffs_proba0"), np.uint8)
UPDATE_PROBA = _table("vp8_coeffs_update_proba")
ENTROPY_COST = _table("vp8_entropy_cost")
CATS = [_table("vp8_cat3"), _table("vp8_cat4"), _table("vp8_cat5"), _table("vp8_cat6")]
assert len(BANDS) == 17 and len(ZIGZAG) == 16 and PROBA0.size == 1056 and len(ENTROPY_COST) == 256

MB_ENC_DTYPE = np.dtype([("coeffs", "<i2", (400,)), ("modes", "u1", (16,)), ("nz_y", "u1", (16,)),
                         ("nz_uv", "u1", (8,)), ("non_zero_y", "<u4"), ("non_zero_uv", "<u4"),
                         ("mb_type", "u1"), ("i16_mode", "u1"), ("uv_mode", "u1"), ("nz_dc", "u1"),
                         ("skip", "u1"), ("segment", "u1"), ("pad", "u1", (2,)), ("score", "<u8")])  # wg_mb_enc
MB_HDR_DTYPE = np.dtype([("modes", "u1", (16,)), ("mb_type", "u1"), ("i16_mode", "u1"), ("uv_mode", "u1"),
                         ("skip", "u1"), ("segment", "u1"), ("pad", "u1", (3,)), ("tok_start", "<u4"),
                         ("tok_count", "<u4")])  # wg_mb_hdr
TOKEN_SUMMARY_DTYPE = np.dtype([("total_tokens", "<u4"), ("num_skip", "<u4"), ("num_updates", "<u4"),
                                ("skip_proba", "u1"), ("pad", "u1", (3,))])  # wg_token_summary
assert MB_ENC_DTYPE.itemsize == 864 and MB_HDR_DTYPE.itemsize == 32 and TOKEN_SUMMARY_DTYPE.itemsize == 16


def bit_cost(bit, prob):
    """dsp.VP8BitCost (internal/dsp/cost.go:43-48)."""
    return ENTROPY_COST[prob] if bit == 0 else ENTROPY_COST[255 - prob]


# --- statistics (encode_proba.go:10-113); stats is a [4][8][3][11][2] nested list ----

def collect_level_stats(level, st):
    """collectLevelStats (:66-113); st = stats[type][band][ctx]."""
    if level == 1:
        st[2][0] += 1
        return
    st[2][1] += 1
    if level <= 4:
        st[3][0] += 1
        if level == 2:
            st[4][0] += 1
        else:
            st[4][1] += 1
            st[5][0 if level == 3 else 1] += 1
    elif level <= 10:
        st[3][1] += 1
        st[6][0] += 1
        st[7][0 if level <= 6 else 1] += 1
    else:
        st[3][1] += 1
        st[6][1] += 1
        cat = 0 if level <= 18 else (1 if level <= 34 else (2 if level <= 66 else 3))
        bit1, bit0 = cat >> 1, cat & 1
        st[8][bit1] += 1
        st[9 + bit1][bit0] += 1


def collect_coeff_stats(coeffs, n_coeffs, ctype, first, ctx, stats):
    """collectCoeffStats (:10-63)."""
    n = first
    if n_coeffs <= first:
        stats[ctype][BANDS[n]][ctx][0][0] += 1
        return
    while n < 16:
        b = BANDS[n]
        if n >= n_coeffs:
            stats[ctype][b][ctx][0][0] += 1
            return
        stats[ctype][b][ctx][0][1] += 1
        while True:
            v = abs(int(coeffs[ZIGZAG[n]]))
            b = BANDS[n]
            if v == 0:
                stats[ctype][b][ctx][1][0] += 1
                n += 1
                if n >= 16:
                    return
                ctx = 0
                continue
            stats[ctype][b][ctx][1][1] += 1
            collect_level_stats(v, stats[ctype][b][ctx])
            ctx = 1 if v == 1 else 2
            n += 1
            break


# --- tokens (encode_token.go:115-300); tokens is a flat list bit, prob, bit, prob ... ----

def record_level(level, p, tokens):
    """recordLevelVP8 (:206-300); p = the 11 probabilities of the band / context."""
    t = tokens.extend
    if level == 1:
        t((0, p[2]))
        return
    t((1, p[2]))
    if level <= 4:
        t((0, p[3]))
        if level == 2:
            t((0, p[4]))
        else:
            t((1, p[4]))
            t((0 if level == 3 else 1, p[5]))
    elif level <= 10:
        t((1, p[3]))
        t((0, p[6]))
        if level <= 6:
            t((0, p[7]))
            t((level - 5, 159))
        else:
            t((1, p[7]))
            v = level - 7
            t((v >> 1, 165))
            t((v & 1, 145))
    else:
        t((1, p[3]))
        t((1, p[6]))
        cat = 0 if level <= 18 else (1 if level <= 34 else (2 if level <= 66 else 3))
        bit1, bit0 = cat >> 1, cat & 1
        t((bit1, p[8]))
        t((bit0, p[9 + bit1]))
        v = level - (3 + (8 << cat))
        tab = CATS[cat]
        nbits = 0
        while tab[nbits] != 0:
            nbits += 1
        for i in range(nbits):
            t(((v >> (nbits - 1 - i)) & 1, tab[i]))


def record_coeffs(coeffs, n_coeffs, ctype, proba, first, ctx, tokens):
    """RecordCoeffs (:115-188); proba indexed [type][band][ctx][11]."""
    n = first
    if n_coeffs <= first:
        tokens.extend((0, proba[ctype][BANDS[n]][ctx][0]))
        return
    while n < 16:
        p = proba[ctype][BANDS[n]][ctx]
        if n >= n_coeffs:
            tokens.extend((0, p[0]))
            return
        tokens.extend((1, p[0]))
        while True:
            v = int(coeffs[ZIGZAG[n]])
            sign = 0
            if v < 0:
                v, sign = -v, 1
            if v == 0:
                tokens.extend((0, p[1]))
                n += 1
                if n >= 16:
                    return
                p = proba[ctype][BANDS[n]][0]
                continue
            tokens.extend((1, p[1]))
            record_level(v, p, tokens)
            tokens.extend((sign, 128))
            ctx = 1 if v == 1 else 2
            n += 1
            break


def _walk_mb(info, top_nz, left_nz, top_nz_dc, left_nz_dc, block):
    """The block walk shared by recordMBTokens (encode_frame.go:647-759) and
    collectMBStats (encode_parallel.go:1602-1707): calls block(coeffs16,
    n_coeffs, type, first, ctx) in the order both use and returns the updated
    (top_nz, left_nz, top_nz_dc, left_nz_dc)."""
    co = info["coeffs"]
    if info["mb_type"] == 0:
        dc_ctx = min(top_nz_dc + left_nz_dc, 2)
        nz_dc = int(info["nz_dc"])
        block(co[384:400], nz_dc, 1, 0, dc_ctx)
        top_nz_dc = left_nz_dc = 1 if nz_dc > 0 else 0
        ctype, first = 0, 1
    else:
        ctype, first = 3, 0
    tnz, lnz = top_nz & 0x0f, left_nz & 0x0f
    for y in range(4):
        l = lnz & 1  # noqa: E741
        for x in range(4):
            b = y * 4 + x
            ctx = min(l + (tnz & 1), 2)
            nz = int(info["nz_y"][b])
            block(co[b * 16:b * 16 + 16], nz, ctype, first, ctx)
            l = 1 if nz > first else 0  # noqa: E741
            tnz = (tnz >> 1) | (l << 7)
        tnz >>= 4
        lnz = (lnz >> 1) | (l << 7)
    out_t, out_l = tnz, lnz >> 4
    for ch in (0, 2):
        tnz, lnz = (top_nz >> (4 + ch)) & 0x0f, (left_nz >> (4 + ch)) & 0x0f
        for y in range(2):
            l = lnz & 1  # noqa: E741
            for x in range(2):
                k = (ch // 2) * 4 + y * 2 + x
                ctx = min(l + (tnz & 1), 2)
                nz = int(info["nz_uv"][k])
                block(co[(16 + k) * 16:(17 + k) * 16], nz, 2, 0, ctx)
                l = 1 if nz > 0 else 0  # noqa: E741
                tnz = (tnz >> 1) | (l << 3)
            tnz >>= 2
            lnz = (lnz >> 1) | (l << 5)
        out_t |= (tnz << 4) << ch
        out_l |= (lnz & 0xf0) << ch
    return out_t, out_l, top_nz_dc, left_nz_dc


def _frame_walk(enc, mbw, mbh, on_mb):
    """The frame loop of collectAllStats (encode_proba.go:171-313) and
    rerecordAllTokens (:317-353): resets, the skipped-MB rule (:193-201,
    :337-345) and the per-MB walk; on_mb(idx) returns the block callback."""
    top_nz, top_nz_dc = [0] * mbw, [0] * mbw
    for y in range(mbh):
        left_nz = left_nz_dc = 0
        for x in range(mbw):
            idx = y * mbw + x
            info = enc[idx]
            if info["skip"]:
                top_nz[x] = 0
                left_nz = 0
                if info["mb_type"] == 0:
                    top_nz_dc[x] = 0
                    left_nz_dc = 0
                on_mb(idx, True)
                continue
            block = on_mb(idx, False)
            top_nz[x], left_nz, top_nz_dc[x], left_nz_dc = _walk_mb(info, top_nz[x], left_nz, top_nz_dc[x], left_nz_dc,
                                                                    block)


def collect_all_stats(enc, mbw, mbh):
    stats = [[[[[0, 0] for _ in range(11)] for _ in range(3)] for _ in range(8)] for _ in range(4)]

    def on_mb(idx, skipped):
        return lambda co, nz, t, first, ctx: collect_coeff_stats(co, nz, t, first, ctx, stats)

    _frame_walk(enc, mbw, mbh, on_mb)
    return np.array(stats, np.int64)


def branch_cost(cnt0, cnt1, proba):
    """branchCost (encode_proba.go:160-168)."""
    proba = min(max(proba, 1), 255)
    return cnt1 * bit_cost(1, proba) + cnt0 * bit_cost(0, proba)


def optimize_proba(stats, proba):
    """optimizeProba (:117-156): proba (1056,) uint8 is updated in place; returns the number of updates."""
    st = stats.reshape(1056, 2)
    updates = 0
    for k in range(1056):
        cnt0, cnt1 = int(st[k, 0]), int(st[k, 1])
        total = cnt0 + cnt1
        if total == 0:
            continue
        new_p = 255 - cnt1 * 255 // total if cnt1 > 0 else 255
        old_p = int(PROBA0[k])
        upd = UPDATE_PROBA[k]
        old_cost = branch_cost(cnt0, cnt1, old_p) + bit_cost(0, upd)
        new_cost = branch_cost(cnt0, cnt1, new_p) + bit_cost(1, upd) + 8 * 256
        if old_cost > new_cost:
            proba[k] = new_p
            updates += 1
    return updates


def record_all_tokens(enc, mbw, mbh, proba):
    """rerecordAllTokens with MarkMBStart (encode_token.go:89-91): (tokens uint8, tok_start, tok_count)."""
    p4 = [[[[int(v) for v in c] for c in b] for b in t] for t in np.asarray(proba).reshape(4, 8, 3, 11)]
    tokens = []
    start = np.zeros(mbw * mbh, np.int64)
    count = np.zeros(mbw * mbh, np.int64)
    state = {"idx": -1}

    def on_mb(idx, skipped):
        if state["idx"] >= 0:
            count[state["idx"]] = len(tokens) // 2 - start[state["idx"]]
        start[idx] = len(tokens) // 2
        state["idx"] = idx
        return lambda co, nz, t, first, ctx: record_coeffs(co, nz, t, p4, first, ctx, tokens)

    _frame_walk(enc, mbw, mbh, on_mb)
    if state["idx"] >= 0:
        count[state["idx"]] = len(tokens) // 2 - start[state["idx"]]
    return np.array(tokens, np.uint8), start, count


def phase_b(enc, mbw, mbh, proba_in=None):
    """What EncodeFrame leaves after Phase B for !doSearch (encode.go:1356-1385):
    dict(stats (4, 8, 3, 11, 2) int64, proba (1056,) uint8, hdr MB_HDR_DTYPE
    (mbh*mbw,), summary TOKEN_SUMMARY_DTYPE (1,), tokens uint8)."""
    enc = np.asarray(enc).reshape(-1)
    assert enc.size == mbw * mbh
    stats = collect_all_stats(enc, mbw, mbh)
    proba = np.array(PROBA0 if proba_in is None else proba_in, np.uint8).reshape(1056).copy()
    updates = optimize_proba(stats, proba)
    tokens, start, count = record_all_tokens(enc, mbw, mbh, proba)
    hdr = np.zeros(enc.size, MB_HDR_DTYPE)
    for f in ("modes", "mb_type", "i16_mode", "uv_mode", "skip", "segment"):
        hdr[f] = enc[f]
    hdr["tok_start"], hdr["tok_count"] = start, count
    total_mb = enc.size
    num_skip = int((enc["skip"] != 0).sum())
    summary = np.zeros(1, TOKEN_SUMMARY_DTYPE)
    summary["total_tokens"] = tokens.size // 2
    summary["num_skip"] = num_skip
    summary["num_updates"] = updates
    if num_skip > 0:  # encode_parallel.go:1595-1597
        summary["skip_proba"] = ((total_mb - num_skip) * 255 // total_mb) & 0xff
    return dict(stats=stats, proba=proba, hdr=hdr, summary=summary, tokens=tokens)


# --- synthetic records -----------------------------------------------------------

# one representative range per branch of recordLevelVP8 (and the zero)
_LEVEL_RANGES = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 6), (7, 10), (11, 18), (19, 34), (35, 66), (67, 2047)]


def _block(rng, first, kind):
    """16 levels in raster order and the zigzag non-zero count (1 + the last
    non-zero zigzag index, 0 for none; positions below `first` stay zero)."""
    lv = np.zeros(16, np.int64)
    if kind == 0:    # all zero
        last = -1
    elif kind == 1:  # runs to position 16: no end-of-block symbol
        last = 15
    else:
        last = int(rng.integers(first, 16))
    for n in range(first, last + 1):
        if n == last or rng.random() < 0.6:
            lo, hi = _LEVEL_RANGES[int(rng.integers(0, len(_LEVEL_RANGES)))]
            mag = int(rng.integers(lo, hi + 1))
            lv[ZIGZAG[n]] = -mag if rng.random() < 0.5 else mag
    return lv, last + 1


def synthetic_records(mbw, mbh, seed):
    """mbw x mbh self-consistent wg_mb_enc records: mixed I16 / I4, skipped MBs
    of both types, every level branch and both signs, all-zero blocks, blocks
    that end at position 16, I16 MBs with nz_dc 0 and non-zero, and (from 3
    rows / columns up) I4 MBs lying between two I16 MBs in a column and a row."""
    rng = np.random.default_rng(seed)
    n = mbw * mbh
    enc = np.zeros(n, MB_ENC_DTYPE)
    mb_type = rng.integers(0, 2, n).astype(np.uint8)
    if mbw >= 3:      # row 0: I16, I4, I16 with distinct DC bits either side
        mb_type[0:3] = (0, 1, 0)
    if mbh >= 3:      # column 0: I16, I4, I16
        mb_type[0], mb_type[mbw], mb_type[2 * mbw] = 0, 1, 0
    skip = rng.random(n) < 0.2
    if n >= 9:
        skip[[0, 1, 2, mbw, 2 * mbw if mbh >= 3 else 0]] = False
    for i in range(n):
        e = enc[i]
        i16 = mb_type[i] == 0
        e["mb_type"] = mb_type[i]
        e["i16_mode"] = rng.integers(0, 4) if i16 else 0
        e["uv_mode"] = rng.integers(0, 4)
        e["segment"] = rng.integers(0, 4)
        if not i16:
            e["modes"] = rng.integers(0, 10, 16)
        if skip[i]:     # a skipped MB: no levels (encode_frame.go: Skip = no non-zero block)
            e["skip"] = 1
            continue
        first = 1 if i16 else 0
        nzy = nzuv = 0
        for b in range(24):
            f = first if b < 16 else 0
            lv, nz = _block(rng, f, int(rng.integers(0, 5)))
            e["coeffs"][b * 16:b * 16 + 16] = lv
            if b < 16:
                e["nz_y"][b] = nz
                nzy |= int(nz > f) << b
            else:
                e["nz_uv"][b - 16] = nz
                nzuv |= int(nz > 0) << (b - 16)
        if i16:
            kind = 0 if (i == 0 or rng.random() < 0.3) else int(rng.integers(1, 5))
            if i == 2:
                kind = 2
            lv, nz = _block(rng, 0, kind)
            e["coeffs"][384:400] = lv
            e["nz_dc"] = nz
            nzy |= int(nz > 0) << 24
        e["non_zero_y"], e["non_zero_uv"] = nzy, nzuv
    return enc
