"""Host geometry and refusal codes of the launchers in pn2_tail.hip, pn2_eval.hip, pn2_input.hip, pn2_zoom.hip and pn2_seg.hip, pinned against a recorded
fixture (the sibling of test_launch_select_cpu.py for these five files).

A fixed sweep goes through the host-only exports (block counts, work sizes, the ragged plan's header, the tail's scratch sizes and its one-pass test) and
through every launching entry point with argument sets that return BEFORE any launch or memset: each pointer null in turn, each shape or range rule broken
in turn, an unknown dtype or element code alone and together with a broken rule (which pins the order of the two), and the `0` returns of empty batches.
Every result must equal tests/golden/launch_select_tail.json, which is recorded with the same sweep from a library build that is known good (PN2_LIB
selects the build):

    PN2_LIB=/path/to/libpn2_hip.so python tests/test_launch_select_tail_cpu.py --record

A change of the launch code that keeps behaviour leaves this test green without re-recording.  The tail's geometry reads PN2_TAIL_BAND: the sweep sets it
to 0 and 1 itself and records the unset case from the environment, so the tests skip when the variable is set outside."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_select_tail.json")
if __name__ == "__main__":          # (under pytest, conftest.py has set the path)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "pranet-v2_amd")]

ENV_SWITCH = "PN2_TAIL_BAND"
PTR = C.c_void_p(4096)            # a non-null, 16-byte aligned pointer for calls that are refused before anything reads it
ODD = C.c_void_p(4100)            # ... and one that is not 16-byte aligned
DTYPES = (0, 1, 2, 3, 7)          # PN2_F32, PN2_BF16, two codes only the conv entry points take, and a code the library does not know
FILES = ("tail", "eval", "input", "zoom", "seg")
INT_MAX = 2 ** 31 - 1


class EvalImg(C.Structure):          # pn2_eval_img
    _fields_ = [("H", C.c_int), ("W", C.c_int), ("off", C.c_longlong), ("rh", C.c_float), ("rw", C.c_float)]


class InputSlot(C.Structure):          # pn2_input_slot
    _fields_ = [(n, C.c_int) for n in ("H", "W", "C", "dst", "norm", "kw", "kh", "blk")] + [(n, C.c_longlong) for n in ("src", "tmp", "tap_w", "tap_h")]


class InputAug(C.Structure):          # pn2_input_aug
    _fields_ = [("a", C.c_int * 6), ("mode", C.c_int), ("reserved", C.c_int)]


def refusals(fn, base, nulls=(), bad=()):
    """fn with each pointer of `nulls` (positions) null in turn, then with each edit of `bad` ({position: value}); `base` itself is never called"""
    r = [fn(*[None if i == p else a for i, a in enumerate(base)]) for p in nulls]
    return r + [fn(*[e.get(i, a) for i, a in enumerate(base)]) for e in bad]


# ------------------------------------------------------------------------------------------------ the tail's descriptors
def tail_desc(capi, sizes, N=2, OH=64, OW=64, P=None, ac=0, ratio=None, dsrc=True, src=True):
    """sizes: (h, w) of maps[0 .. 2P); ratio: (rh, rw) instead of the bilinear ones"""
    d = capi.TailDesc()
    d.N, d.OH, d.OW, d.P, d.align_corners = N, OH, OW, len(sizes) // 2 if P is None else P, ac
    for j, (h, w) in enumerate(sizes):
        m = d.maps[j]
        m.src, m.dsrc, m.h, m.w = (PTR if src else None), (PTR if dsrc else None), h, w
        if ratio:
            m.rh, m.rw = ratio
        elif ac:
            m.rh, m.rw = ((h - 1) / (OH - 1) if OH > 1 else 0.0), ((w - 1) / (OW - 1) if OW > 1 else 0.0)
        else:
            m.rh, m.rw = h / OH, w / OW
    return d


def square(S, mags):
    """maps of S / mag pixels a side: pair p = (maps[p], maps[P + p]) of one magnification"""
    return [(S // m, S // m) for m in mags] * 2


def tail_geometry(capi, lib):
    r = []
    descs = []
    for S in (64, 352, 512, 640):
        for P in (1, 2, 3, 4):
            for ac in (0, 1):
                descs.append(tail_desc(capi, square(S, (8, 16, 32, 32)[:P]), OH=S, OW=S, ac=ac))           # the one-pass geometry where S allows it
                descs.append(tail_desc(capi, square(S, (16, 16, 16, 16)[:P]), OH=S, OW=S, ac=ac, N=5))
        descs.append(tail_desc(capi, square(S, (2, 2)), OH=S, OW=S))                                      # magnification 2: a band touches more than 3 rows
        descs.append(tail_desc(capi, square(S, (4, 8)), OH=S, OW=S))                                      # magnification 4: band kernels, not the one-pass one
        descs.append(tail_desc(capi, [(S // 8, S // 8), (S // 16, S // 16), (S // 16, S // 16), (S // 8, S // 8)], OH=S, OW=S))      # pairs of unequal geometry
        descs.append(tail_desc(capi, [(S // 8, S // 8), (S // 8, S // 16)], OH=S, OW=S))
    descs.append(tail_desc(capi, [(32, 32)] * 4, OH=352, OW=352))                                         # magnification 11
    descs.append(tail_desc(capi, [(20, 20)] * 2, OH=100, OW=100))                                         # 5, and a ragged last band
    descs.append(tail_desc(capi, [(2, 2)] * 2, OH=64, OW=64))                                             # maps of fewer than 5 pixels
    descs.append(tail_desc(capi, square(64, (8,)), OH=64, OW=64, N=512))
    descs.append(tail_desc(capi, square(64, (8,)), OH=64, OW=64, N=513))                                  # tail_check: P * N > 512
    descs.append(tail_desc(capi, square(64, (8,)), OH=64, OW=66))                                         # OW no multiple of 4
    descs.append(tail_desc(capi, square(64, (8,)), OH=64, OW=64, P=0))
    descs.append(tail_desc(capi, square(64, (8, 8, 8, 8, 8)), OH=64, OW=64))                              # P = 5
    descs.append(tail_desc(capi, square(64, (8,)), OH=64, OW=64, src=False))
    for env in (None, "0", "1"):
        if env is None:
            os.environ.pop(ENV_SWITCH, None)
        else:
            os.environ[ENV_SWITCH] = env
        r += [[lib.pn2_dsra_tail_scratch(C.byref(d)), lib.pn2_dsra_tail_fused_ok(C.byref(d)), lib.pn2_dsra_tail_fused_scratch(C.byref(d))] for d in descs]
        r.append([lib.pn2_dsra_tail_scratch(None), lib.pn2_dsra_tail_fused_ok(None), lib.pn2_dsra_tail_fused_scratch(None)])
    os.environ.pop(ENV_SWITCH, None)
    return r


def tail_refusals(capi, lib):
    r = []
    r += refusals(lib.pn2_dsra_fuse_fwd, [PTR, PTR, PTR, PTR, 4096, 8, 1, None], nulls=range(4), bad=[{5: 33}, {5: 33, 0: None}])
    r += refusals(lib.pn2_dsra_fuse_bwd, [PTR] * 7 + [4096, 8, 1, None], nulls=range(7), bad=[{8: 33}, {8: 33, 6: None}])
    for dt in DTYPES:          # C and every ld are tested against 8 for fp32 as well
        fwd = [dt, PTR, 64, PTR, PTR, 64, 4096, 64, None]
        bwd = [dt, PTR, 64, PTR, PTR, 64, PTR, 64, 0, PTR, 4096, 64, None]
        post = [dt, PTR, 64, PTR, PTR, 64, PTR, 64, PTR, 4096, 64, None]
        r += refusals(lib.pn2_ra_gate_fwd, fwd, nulls=(1, 3, 4), bad=[{7: 68}, {7: 4}, {2: 68}, {5: 68}, {7: 68, 1: None}])
        r += refusals(lib.pn2_ra_gate_bwd, bwd, nulls=(1, 3, 4, 6, 9), bad=[{11: 68}, {11: 4}, {2: 68}, {5: 68}, {7: 68}])
        r += refusals(lib.pn2_ra_gate_post_bwd, post, nulls=(1, 3, 4, 6, 8), bad=[{10: 68}, {10: 4}, {2: 68}, {5: 68}, {7: 68}])
        if dt not in (0, 1):
            r += [lib.pn2_ra_gate_fwd(*fwd), lib.pn2_ra_gate_bwd(*bwd), lib.pn2_ra_gate_post_bwd(*post)]
    r += refusals(lib.pn2_loss_weights_clear, [PTR, PTR, 2, 64, 64, 31, PTR, 10, None], nulls=(0, 1, 6),
                  bad=[{7: -1}, {5: 0}, {5: 30}, {5: 65}, {5: -3}, {5: 30, 0: None}, {6: None, 7: 0, 5: 64}])
    r += refusals(lib.pn2_loss_weights, [PTR, PTR, 2, 64, 64, 31, None], nulls=(0, 1), bad=[{5: 0}, {5: 30}, {5: 65}])
    r += refusals(lib.pn2_structure_loss_fwd, [PTR, 4096, 4, PTR, PTR, PTR, PTR, PTR, PTR, 2, 4096, None], nulls=(0, 3, 4, 5, 6, 7, 8),
                  bad=[{2: 9, 9: 1}, {9: 129}, {2: 8, 9: 65}, {9: 129, 0: None}])
    r += refusals(lib.pn2_structure_loss_bwd, [PTR, PTR, 4096, 4, PTR, PTR, PTR, PTR, 1.0, 2, 4096, None], nulls=(0, 1, 4, 5, 6, 7))
    r += refusals(lib.pn2_structure_loss_bwd_dev, [PTR, PTR, 4096, 4096, 4, PTR, PTR, PTR, PTR, None, 1.0, 2, 4096, None], nulls=(0, 1, 5, 6, 7, 8),
                  bad=[{2: -1}, {3: -1}, {2: -1, 0: None}])
    r += refusals(lib.pn2_adam_tick, [PTR, 0.9, 0.999, None], nulls=(0,))
    r += refusals(lib.pn2_clamp_adam, [PTR, PTR, PTR, PTR, 1000, 1e-4, 0.9, 0.999, 1e-8, 0.5, 1.0, PTR, 0.0, None], nulls=(0, 1, 2, 3, 11),
                  bad=[{0: ODD}, {1: ODD}, {2: ODD}, {3: ODD}, {0: ODD, 11: None}])
    r += refusals(lib.pn2_eval_tail, [PTR, PTR, PTR, 4096, None], nulls=(0, 1, 2))
    r += refusals(lib.pn2_eval_hist, [PTR, PTR, 4096, PTR, None], nulls=(0, 1, 3), bad=[{2: 0}, {2: -5}])

    ok = tail_desc(capi, square(64, (8, 16)))
    huge = tail_desc(capi, square(64, (8, 16)), ratio=(1000.0, 0.125))          # row kernels whose LDS need is above the 60 KiB they accept
    broken = [tail_desc(capi, square(64, (8,)), P=0), tail_desc(capi, square(64, (8, 8, 8, 8, 8))), tail_desc(capi, square(64, (8,)), OW=66),
              tail_desc(capi, square(64, (8,)), OW=1028, OH=1028), tail_desc(capi, square(64, (8,)), N=0), tail_desc(capi, square(64, (8,)), N=513),
              tail_desc(capi, square(64, (8,)), src=False), tail_desc(capi, [(0, 8), (8, 8)]), tail_desc(capi, [(8, 0), (8, 8)]), tail_desc(capi, [(8, 65), (8, 8)]),
              tail_desc(capi, [(65, 8), (8, 8)])]
    nosrc = tail_desc(capi, square(64, (8, 16)), dsrc=False)
    ref = C.byref
    fwd = lambda d, **n: lib.pn2_dsra_tail_fwd(d, *[None if k in n else PTR for k in ("lat", "mask", "weit", "partial", "sums", "wsum", "loss")], None)
    bwd = lambda d, **n: lib.pn2_dsra_tail_bwd(d, *[None if k in n else PTR for k in ("mask", "weit", "wsum", "sums")], 1.0, None, 0, None)
    one = lambda d, floats=1 << 40, **n: lib.pn2_dsra_tail_fwd_bwd(
        d, *[None if k in n else PTR for k in ("lat", "mask", "weit", "partial", "sums", "wsum", "per", "loss")], 1.0, None if "scratch" in n else PTR, floats, None, None)
    for env in (None, "0", "1"):
        if env is None:
            os.environ.pop(ENV_SWITCH, None)
        else:
            os.environ[ENV_SWITCH] = env
        r += [fwd(ref(ok), **{k: 1}) for k in ("lat", "mask", "weit", "partial", "sums", "wsum", "loss")] + [fwd(None), fwd(None, lat=1), fwd(ref(huge))]
        r += [fwd(ref(d)) for d in broken]
        r += [bwd(ref(ok), **{k: 1}) for k in ("mask", "weit", "wsum", "sums")] + [bwd(None), bwd(None, mask=1), bwd(ref(nosrc)), bwd(ref(huge))]
        r += [bwd(ref(d)) for d in broken]
        r += [one(ref(ok), **{k: 1}) for k in ("lat", "mask", "weit", "partial", "sums", "wsum", "per", "loss", "scratch")] + [one(None), one(None, lat=1), one(ref(nosrc))]
        r += [one(ref(d)) for d in broken]
        # no one-pass geometry: align_corners, OW above 512, magnification 4 and 11, an unequal pair; then a scratch one float short
        r += [one(ref(tail_desc(capi, square(64, (8, 16)), ac=1))), one(ref(tail_desc(capi, square(640, (8, 16)), OH=640, OW=640))), one(ref(tail_desc(capi, square(64, (4, 8))))),
              one(ref(tail_desc(capi, [(32, 32)] * 2, OH=352, OW=352))), one(ref(tail_desc(capi, [(8, 8), (4, 4)]))), one(ref(huge))]
        if env != "0" and env != "1":
            r.append(one(ref(ok), floats=lib.pn2_dsra_tail_fused_scratch(ref(ok)) - 1))
        else:
            r.append(one(ref(ok)))          # PN2_TAIL_BAND = 0 or 1 takes the one-pass kernel away: -2
    os.environ.pop(ENV_SWITCH, None)
    return r


# ------------------------------------------------------------------------------------------------ evaluation
def eval_refusals(capi, lib):
    r = []
    r += refusals(lib.pn2_eval_region_sums, [PTR, PTR, 64, 64, PTR, None], nulls=(0, 1, 4), bad=[{2: 0}, {3: 0}])
    r += refusals(lib.pn2_eval_wfm, [PTR, PTR, 64, 64, PTR, -0.1, PTR, PTR, PTR, None], nulls=(0, 1, 4, 6, 7, 8), bad=[{2: 0}, {3: 0}, {3: 15361}, {3: 15361, 0: None}])
    four = (C.c_void_p * 4)(4096, 4096, 4096, 4096)
    hole = (C.c_void_p * 4)(4096, 4096, None, 4096)
    first = (C.c_void_p * 4)(None, 4096, 4096, 4096)
    # batch_check, given the positions of B, maxH, maxW and total: an empty size (-1), outside the built range (-2), and -1 in front of -2
    batch = lambda b, mh, mw, tot: [{b: 0}, {mh: 0}, {mw: 0}, {tot: 0}, {b: 65536}, {mw: 15361}, {b: 65536, mh: 0}]
    r += refusals(lib.pn2_eval_tail_batch, [four, 4, 8, 11, 11, PTR, 352, 352, 8 * 352 * 352, PTR, PTR, None], nulls=(0, 5, 9, 10),
                  bad=batch(2, 6, 7, 8) + [{3: 0}, {4: 0}, {1: 0}, {1: 2}, {1: 3}, {1: 5}, {3: 32768, 4: 32768}, {0: hole}, {0: first, 1: 1}, {1: 2, 2: 65536},
                                           {0: hole, 1: 3}])
    r += refusals(lib.pn2_eval_counts_batch, [PTR, PTR, PTR, 8, 352, 352, 8 * 352 * 352, PTR, PTR, None], nulls=(0, 1, 2, 7), bad=batch(3, 4, 5, 6) + [{7: None, 3: 65536}])
    r += refusals(lib.pn2_eval_wfm_batch, [PTR, PTR, PTR, 8, 352, 352, 8 * 352 * 352, PTR, -0.1, PTR, PTR, PTR, None], nulls=(0, 1, 2, 7, 9, 10, 11),
                  bad=batch(3, 4, 5, 6) + [{7: None, 3: 65536}])
    return r


# ------------------------------------------------------------------------------------------------ input transform
def slots(lib, rows, S=32, **edit):
    """a valid table of len(rows) slots ((H, W, C) each; H = 0: empty) with packed arenas; edit: field = (slot, value)"""
    t = (InputSlot * max(len(rows), 1))()
    src = tmp = tap = blk = 0
    dst = {1: 0, 3: 0}
    for i, (H, W, Cn) in enumerate(rows):
        s = t[i]
        s.H, s.W, s.C, s.blk = H, W, Cn, blk
        if H == 0:
            continue
        s.dst, s.norm, s.src, s.tmp = dst[Cn], 1, src, tmp
        dst[Cn] += 1
        s.kw, s.kh = lib.pn2_resize_ksize(W, S), lib.pn2_resize_ksize(H, S)
        s.tap_w, s.tap_h = tap, tap + 2 * S + S * s.kw
        tap += 4 * S + S * (s.kw + s.kh)
        src += H * W * Cn
        tmp += (H * S * Cn + 3) & ~3
        blk += lib.pn2_input_batch_blocks(H, S)
    for k, (i, v) in edit.items():
        setattr(t[i], k, v)
    return t, src, tmp, tap, dst[3], dst[1]


def input_refusals(capi, lib):
    r = []
    r += refusals(lib.pn2_resize_u8_pass, [PTR, PTR, 64, 64, 3, 32, 1, PTR, PTR, PTR, 5, None], nulls=(0, 1, 7, 8, 9), bad=[{2: 0}, {3: 0}, {4: 0}, {5: 0}, {6: 2}, {6: -1}])
    r += refusals(lib.pn2_u8_to_tensor, [PTR, PTR, 64, 64, 3, PTR, PTR, None], nulls=(0, 1, 5, 6), bad=[{2: 0}, {3: 0}, {4: 0}])
    rows = [(40, 50, 3), (40, 50, 1), (0, 0, 0), (32, 32, 3), (17, 90, 1)]
    S = 32
    # a table edit and the passes that check the field ("w": width, "a": width with the second table, "h": height)
    both, wid_only, hei_only = "wah", "wa", "h"
    edits = [({}, both), (dict(H=(0, -1)), both), (dict(W=(1, 0)), both), (dict(blk=(1, 0)), both), (dict(C=(0, 2)), both), (dict(src=(1, -1)), wid_only), (dict(src=(4, 1 << 40)), wid_only),
             (dict(tmp=(0, -4)), both), (dict(tmp=(4, 1 << 40)), both), (dict(kw=(0, 7)), wid_only), (dict(tap_w=(0, -1)), wid_only), (dict(tap_w=(4, 1 << 40)), wid_only),
             (dict(kh=(0, 7)), hei_only), (dict(tap_h=(0, -1)), hei_only), (dict(tap_h=(4, 1 << 40)), hei_only), (dict(dst=(0, -1)), hei_only), (dict(dst=(0, 2)), hei_only),
             (dict(dst=(1, 2)), hei_only), (dict(H=(0, 1 << 17), W=(0, 1 << 16)), wid_only), (dict(H=(0, 1 << 26)), both)]
    aug = (InputAug * len(rows))()
    for i in range(len(rows)):
        aug[i].mode = i & 1
        aug[i].a[0] = aug[i].a[4] = 65536
    for e, passes in edits:
        t, src, tmp, tap, n_rgb, n_mask = slots(lib, rows, S, **e)
        wid = [t, PTR, len(rows), S, PTR, src, PTR, tmp, PTR, tap, None]
        wau = [t, PTR, aug, PTR, len(rows), S, PTR, src, PTR, tmp, PTR, tap, None]
        hei = [t, PTR, len(rows), S, PTR, tmp, PTR, tap, PTR, n_rgb, PTR, n_mask, PTR, PTR, None]
        if not e:          # the valid table: nulls, scalar rules and the returns of 0 (these return before the table's walk ends in a launch)
            r += refusals(lib.pn2_input_batch_width, wid, nulls=(0, 1, 4, 6, 8), bad=[{2: -1}, {3: 0}, {5: -1}, {7: -1}, {9: -1}, {2: 0}, {2: 0, 0: None}, {3: 46341}, {5: src - 1},
                                                                                     {7: tmp - 1}, {9: 10}])
            r += refusals(lib.pn2_input_batch_width_aug, wau, nulls=(0, 1, 2, 3, 6, 8, 10), bad=[{4: -1}, {5: 0}, {7: -1}, {9: -1}, {11: -1}, {4: 0}, {4: 0, 2: None}, {5: 46341},
                                                                                                {7: src - 1}, {9: tmp - 1}, {11: 10}])
            r += refusals(lib.pn2_input_batch_height, hei, nulls=(0, 1, 4, 6, 8, 10, 12, 13), bad=[{2: -1}, {3: 0}, {5: -1}, {7: -1}, {9: -1}, {11: -1}, {2: 0}, {2: 0, 12: None}, {3: 46341},
                                                                                                  {5: tmp - 1}, {7: tap - 1}, {9: n_rgb - 1}, {11: n_mask - 1}])
        else:
            r += [fn(*a) for fn, a, k in ((lib.pn2_input_batch_width, wid, "w"), (lib.pn2_input_batch_width_aug, wau, "a"), (lib.pn2_input_batch_height, hei, "h")) if k in passes]
    # every slot empty: 0 before any launch
    t, src, tmp, tap, n_rgb, n_mask = slots(lib, [(0, 0, 0)] * 3, S)
    r += [lib.pn2_input_batch_width(t, PTR, 3, S, PTR, 0, PTR, 0, PTR, 0, None), lib.pn2_input_batch_width_aug(t, PTR, aug, PTR, 3, S, PTR, 0, PTR, 0, PTR, 0, None),
          lib.pn2_input_batch_height(t, PTR, 3, S, PTR, 0, PTR, 0, None, 0, None, 0, PTR, PTR, None)]
    # the second table: an unknown mode (-3) in front of a table error, an axis above the bound, sums that leave int32
    t, src, tmp, tap, n_rgb, n_mask = slots(lib, rows, S)
    for e in ({"mode": (0, 2)}, {"mode": (4, -1)}, {"a2": (1, INT_MAX)}, {"a0": (1, 1 << 30)}, {"a4": (1, -(1 << 30))}, {"mode": (2, 2)}):
        g = (InputAug * len(rows))()
        for i in range(len(rows)):
            g[i].mode, g[i].a[0], g[i].a[4] = i & 1, 65536, 65536
        for k, (i, v) in e.items():
            if k == "mode":
                g[i].mode = v
            else:
                g[i].a[int(k[1])] = v
        r.append(lib.pn2_input_batch_width_aug(t, PTR, g, PTR, len(rows), S, PTR, src, PTR, tmp, PTR, tap, None))
    bad_t, *_ = slots(lib, rows, S, blk=(1, 0))
    g = (InputAug * len(rows))()
    g[0].mode = 5
    r.append(lib.pn2_input_batch_width_aug(bad_t, PTR, g, PTR, len(rows), S, PTR, src, PTR, tmp, PTR, tap, None))          # check_aug runs first: -3 from the mode
    big, bsrc, btmp, btap, _, _ = slots(lib, [(20000, 8, 1), (8, 8, 1)], S)
    g = (InputAug * 2)()
    g[0].mode = g[1].mode = 1
    r.append(lib.pn2_input_batch_width_aug(big, PTR, g, PTR, 2, S, PTR, bsrc, PTR, btmp, PTR, btap, None))
    # the height pass's grid: blocks per slot x slots above INT_MAX
    n, S2 = 4096, 26000
    t = (InputSlot * n)()
    per = lib.pn2_input_batch_blocks(1, S2)
    for i in range(n):
        t[i].H, t[i].W, t[i].C, t[i].blk, t[i].tmp, t[i].kh, t[i].kw = 1, 1, 1, i * per, i * S2, lib.pn2_resize_ksize(1, S2), lib.pn2_resize_ksize(1, S2)
    r.append(lib.pn2_input_batch_height(t, PTR, n, S2, PTR, n * S2, PTR, 5 * S2, None, 0, PTR, 1, PTR, PTR, None))
    return r


# ------------------------------------------------------------------------------------------------ spline zoom
def plan(capi, lib, samples, packed=1, room=0):
    """(status of pn2_ragged_plan_bound, bound, status of pn2_ragged_plan, header fields) and the blob"""
    n = len(samples)
    arr = (capi.RaggedSample * max(n, 1))()
    for i, s in enumerate(samples):
        for k, v in s.items():
            setattr(arr[i], k, v)
    bound = C.c_longlong(-1)
    rb = lib.pn2_ragged_plan_bound(n, arr, C.byref(bound))
    size = max(int(bound.value), 0) + room
    blob = (C.c_char * max(size, 128))()
    rp = lib.pn2_ragged_plan(n, arr, packed, blob, size)
    h = capi.RaggedHeader.from_buffer_copy(bytes(blob)[:C.sizeof(capi.RaggedHeader)])
    fields = [getattr(h, f) for f, _ in capi.RaggedHeader._fields_] if rp == 0 else []
    return [rb, bound.value, rp, fields], blob


def zoom_geometry(capi, lib, out):
    r = []
    for n in (-1, 0, 1, 2, 1024, 1025):
        z = C.c_double(0.0)
        r.append([lib.pn2_zoom_pole_pow(n, C.byref(z)), z.value.hex()])
    r.append([lib.pn2_zoom_pole_pow(8, None), ""])
    out["zoom_pole_pow"] = r
    r = []
    for a in ((1, 1, 1), (0, 8, 8), (1, 0, 8), (1, 8, 0), (3, 7, 9), (16, 1024, 1024), (1, 1025, 8), (1, 8, 1025), (1 << 20, 1024, 1024), (1 << 20, 1024, 1023), (2, 224, 224)):
        b = C.c_longlong(-1)
        r.append([lib.pn2_zoom_workspace(*a, C.byref(b)), b.value])
    r.append([lib.pn2_zoom_workspace(1, 8, 8, None), -1])
    out["zoom_workspace"] = r
    s = lambda H, W, oh, ow, geom=0, k=0, axis=-1, **kw: dict(H=H, W=W, oh=oh, ow=ow, geom=geom, k=k, axis=axis, **kw)
    sets = [[s(512, 512, 224, 224)], [s(224, 224, 224, 224)], [s(512, 512, 224, 224), s(224, 224, 224, 224), s(300, 400, 224, 224, geom=1, k=1, axis=0)],
            [s(7, 9, 5, 3), s(9, 7, 3, 5, geom=1, k=1), s(7, 9, 5, 3, geom=2)], [s(1, 1, 1, 1)], [s(1024, 1024, 1024, 1024), s(1024, 1024, 1, 1)], [s(100, 100, 50, 60), s(100, 100, 60, 50)],
            [s(0, 8, 8, 8)], [s(8, 8, 0, 8)], [s(1025, 8, 8, 8)], [s(8, 8, 8, 1025)], [s(8, 8, 8, 8, geom=3)], [s(8, 8, 8, 8, geom=1, k=4)], [s(8, 8, 8, 8, geom=1, k=1, axis=2)],
            [s(8, 8, 8, 8, geom=-1)], []]
    r = [plan(capi, lib, x)[0] for x in sets] + [plan(capi, lib, sets[2], packed=0)[0], plan(capi, lib, sets[0], room=-20000)[0]]
    arr = (capi.RaggedSample * 1)()
    b = C.c_longlong(-1)
    r.append([lib.pn2_ragged_plan_bound(1, None, C.byref(b)), lib.pn2_ragged_plan_bound(1, arr, None), lib.pn2_ragged_plan_bound(4097, arr, C.byref(b)),
              lib.pn2_ragged_plan(1, None, 1, PTR, 4096), lib.pn2_ragged_plan(1, arr, 1, None, 4096), lib.pn2_ragged_plan(4097, arr, 1, PTR, 4096)])
    out["ragged_plan"] = r


def zoom_refusals(capi, lib):
    r = []
    big = {1: 1 << 30, 2: 1, 3: 65}          # N * ceil(W / 64) blocks above INT_MAX with N * H * W below 2^40
    r += refusals(lib.pn2_zoom_prefilter, [PTR, 2, 64, 64, PTR, None], nulls=(0, 4), bad=[{1: 0}, {2: 0}, {3: 0}, {2: 1025}, {3: 1025}, big, {1: 1 << 30, 2: 65, 3: 1}, {1: 0, 0: None}])
    r += refusals(lib.pn2_zoom3_gather, [PTR, 2, 64, 64, 32, 32] + [PTR] * 7 + [None], nulls=(0, 6, 7, 8, 9, 10, 11, 12), bad=[{1: 0}, {2: 1025}, {4: 0}, {5: 1025}, {4: 0, 0: None}])
    for elem in (1, 4, 0, 2, 8):
        z0 = [elem, PTR, 2, 64, 64, 32, 32, PTR, PTR, PTR, PTR, PTR, None]
        ro = [elem, PTR, 2, 64, 64, PTR, PTR, None]
        rf = [elem, PTR, 2, 64, PTR, PTR, None]
        r += refusals(lib.pn2_zoom0, z0, nulls=(1, 7, 8, 9, 10, 11), bad=[{2: 0}, {3: 1025}, {5: 0}, {6: 1025}])
        r += refusals(lib.pn2_rotate0, ro, nulls=(1, 5, 6), bad=[{2: 0}, {3: 1025}, {4: 0}])
        r += refusals(lib.pn2_rot_flip, rf, nulls=(1, 4, 5), bad=[{2: 0}, {3: 1025}, {3: 0}])
        if elem not in (1, 4):
            r += [lib.pn2_zoom0(*z0), lib.pn2_rotate0(*ro), lib.pn2_rot_flip(*rf)]
    s = lambda H, W, oh, ow: dict(H=H, W=W, oh=oh, ow=ow, geom=0, k=0, axis=-1)
    _, work = plan(capi, lib, [s(512, 512, 224, 224), s(224, 224, 224, 224)])          # one sample to filter, one copy
    _, copy = plan(capi, lib, [s(224, 224, 224, 224)])                                 # every sample at its output size
    bad = []
    for field, v in (("magic", 0), ("N", 0), ("N", 4097), ("blocks0", -1), ("blocks1", 0), ("max_out", 0), ("max_out", 1024 * 1024 + 1), ("desc_off", 0)):
        b = (C.c_char * len(work)).from_buffer_copy(bytes(work))
        setattr(capi.RaggedHeader.from_buffer(b), field, v)
        bad.append(b)
    r += refusals(lib.pn2_ragged_prefilter, [PTR, work, PTR, PTR, None], nulls=(0, 1, 2, 3)) + [lib.pn2_ragged_prefilter(PTR, b, PTR, PTR, None) for b in bad]
    r += [lib.pn2_ragged_prefilter(PTR, copy, PTR, None, None), lib.pn2_ragged_prefilter(PTR, copy, PTR, PTR, None), lib.pn2_ragged_prefilter(None, copy, PTR, PTR, None)]
    r += refusals(lib.pn2_ragged_zoom3, [PTR, work, PTR, PTR, PTR, None], nulls=(0, 1, 2, 3, 4)) + [lib.pn2_ragged_zoom3(PTR, b, PTR, PTR, PTR, None) for b in bad]
    r += refusals(lib.pn2_ragged_zoom0, [PTR, work, PTR, PTR, None], nulls=(0, 1, 2, 3)) + [lib.pn2_ragged_zoom0(PTR, b, PTR, PTR, None) for b in bad]
    r += refusals(lib.pn2_ragged_dice_counts, [PTR, PTR, work, PTR, PTR, None], nulls=(0, 1, 2, 3, 4)) + [lib.pn2_ragged_dice_counts(PTR, PTR, b, PTR, PTR, None) for b in bad]
    return r


# ------------------------------------------------------------------------------------------------ labels and volume metrics
def seg_geometry(capi, lib, out):
    r = []
    for a in ((1, 8, 8, 2), (1, 8, 8, 3), (4, 8, 8, 2), (4, 8, 8, 3), (0, 8, 8, 3), (4, 0, 8, 3), (4, 8, 0, 3), (1024, 1024, 1024, 3), (1025, 8, 8, 3), (8, 1025, 8, 3), (8, 8, 1025, 3),
              (8, 8, 8, 1), (8, 8, 8, 4), (148, 512, 512, 3)):
        b = C.c_longlong(-1)
        r.append([lib.pn2_seg_surface_workspace(*a, C.byref(b)), b.value, lib.pn2_seg_surface_hist_len(*a[:3])])
    r.append([lib.pn2_seg_surface_workspace(4, 8, 8, 3, None), -1, 0])
    out["seg_surface_sizes"] = r


def seg_refusals(capi, lib):
    r = []
    eight = (C.c_void_p * 8)(*[4096] * 8)
    hole = (C.c_void_p * 8)(4096, None, 4096, 4096, 4096, 4096, 4096, 4096)
    shape = [{2: -1}, {2: 3}, {4: 1}, {4: 17}, {1: 0}, {1: 9}, {2: 2, 1: 3}]
    r += refusals(lib.pn2_seg_labels, [eight, 4, 0, 2, 9, 32, 32, PTR, None], nulls=(0, 7), bad=[{3: 0}, {5: 0}, {6: 0}] + shape + [{0: hole}, {0: hole, 1: 2}, {0: hole, 4: 1}, {4: 1, 7: None}])

    def up(n=4, K=9, **e):
        m = (capi.SegUpMap * 8)()
        for i in range(8):
            m[i].p, m[i].ld, m[i].H, m[i].W = 4096, 12, 8, 8
        for k, (i, v) in e.items():
            setattr(m[i], k, v)
        return m
    base = [up(), 4, 0, 2, 9, 32, 32, PTR, None]
    r += refusals(lib.pn2_seg_labels_up, base, nulls=(0, 7), bad=[{3: 0}, {5: 0}, {6: 0}] + shape + [{3: 65536}, {5: 4 * 65535 + 1, 6: 8}, {4: 1, 7: None}])
    r += [lib.pn2_seg_labels_up(up(**e), 4, 0, 2, 9, 32, 32, PTR, None) for e in (dict(p=(1, None)), dict(ld=(0, 8)), dict(H=(2, 0)), dict(W=(3, 0)), dict(H=(0, 5)), dict(W=(0, 5)),
                                                                                    dict(H=(0, 16)), dict(p=(3, None), ld=(0, 8)), dict(ld=(0, 8), p=(3, None)))]
    r.append(lib.pn2_seg_labels_up(up(p=(3, None)), 4, 3, 2, 9, 32, 32, PTR, None))          # an unknown mode in front of a null map: -2
    r += refusals(lib.pn2_seg_counts, [PTR, PTR, 4096, 9, PTR, None], nulls=(0, 1, 4), bad=[{2: 0}, {3: 0}, {3: 257}, {3: 0, 0: None}])
    r += refusals(lib.pn2_seg_surface_hist, [PTR, PTR, 4, 32, 32, 1, 3, PTR, PTR, PTR, None], nulls=(0, 1, 7, 8, 9),
                  bad=[{2: 0}, {3: 1025}, {4: 0}, {6: 2}, {6: 4}, {5: -1}, {5: 256}, {5: 256, 0: None}])
    return r


def sweep(capi):
    """section name -> list of results, in a fixed order"""
    lib = capi.load()
    out = {}
    out["loss_blocks"] = [lib.pn2_loss_blocks(hw) for hw in (-1, 0, 1, 4095, 4096, 4097, 123904, 262143, 262144, 262145, 1 << 24, INT_MAX - 4095)]
    out["dsra_tail_blocks"] = [lib.pn2_dsra_tail_blocks(oh) for oh in (0, 1, 7, 8, 9, 64, 100, 352, 1024)]
    out["eval_wfm_blocks"] = [lib.pn2_eval_wfm_blocks(h, w) for h, w in ((0, 0), (1, 1), (16, 16), (16, 17), (352, 352), (724, 724), (725, 724), (1024, 1024), (46340, 46340))]
    out["input_batch_blocks"] = [lib.pn2_input_batch_blocks(rows, s) for rows in (-1, 0, 1, 7, 30, 352, 4096, INT_MAX) for s in (0, 1, 3, 4, 30, 32, 352, 1024, INT_MAX)]
    out["tail_geometry"] = tail_geometry(capi, lib)
    zoom_geometry(capi, lib, out)
    seg_geometry(capi, lib, out)
    for f, fn in zip(FILES, (tail_refusals, eval_refusals, input_refusals, zoom_refusals, seg_refusals)):
        out[f"refusals_{f}"] = fn(capi, lib)
    return out


def _load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


pytestmark = pytest.mark.skipif(ENV_SWITCH in os.environ, reason="the sweep is recorded with PN2_TAIL_BAND unset outside")


@pytest.fixture(scope="module")
def results():
    from pn2 import capi
    return sweep(capi)


SECTIONS = ["loss_blocks", "dsra_tail_blocks", "eval_wfm_blocks", "input_batch_blocks", "tail_geometry", "zoom_pole_pow", "zoom_workspace", "ragged_plan", "seg_surface_sizes"] + \
           [f"refusals_{f}" for f in FILES]
# what the refusals of a file consist of: the library's negative codes, and 0 where an empty batch returns before any launch
CODES = {"tail": {-1, -2, -3}, "eval": {-1, -2}, "input": {0, -1, -2, -3}, "zoom": {0, -1, -2, -3}, "seg": {-1, -2}}


def test_sections_complete(results):
    assert sorted(results) == sorted(SECTIONS) == sorted(_load_fixture())


@pytest.mark.parametrize("section", SECTIONS)
def test_plan_matches_recorded(results, section):
    want, got = _load_fixture()[section], json.loads(json.dumps(results[section]))
    assert len(got) == len(want), (section, len(got), len(want))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{section}: {len(bad)} of {len(got)} results differ from the recorded ones; first (index, got, recorded): {bad[:8]}"


@pytest.mark.parametrize("f", FILES)
def test_refusals_never_launch(results, f):
    """a refusal is one of the library's own codes; a HIP error code (positive) would mean that a case reached a launch"""
    assert set(results[f"refusals_{f}"]) == CODES[f], sorted(set(results[f"refusals_{f}"]))


def test_sweep_reaches_every_branch(results):
    g = results["tail_geometry"]
    n = len(g) // 3
    unset, band0, band1 = g[:n], g[n:2 * n], g[2 * n:]
    assert any(r[0] > 0 and r[1] == 1 and r[2] > 0 for r in unset)          # band kernels and the one-pass kernel
    assert any(r[0] > 0 and r[1] == 0 for r in unset) and any(r[0] == 0 for r in unset)          # band kernels only; row kernels
    assert all(r == [0, 0, 0] for r in band0)                               # PN2_TAIL_BAND=0: row kernels everywhere
    assert any(r[0] > 0 for r in band1) and all(r[1:] == [0, 0] for r in band1)          # =1: band kernels, never the one-pass kernel
    assert [r[0] for r in band1] == [r[0] for r in unset]
    plans = results["ragged_plan"]
    assert {p[2] for p in plans[:-1]} == {0, -2, -3, -4} and any(p[3] and p[3][2] == 0 for p in plans[:-1]) and any(p[3] and p[3][2] > 0 for p in plans[:-1])
    assert -1 in results["input_batch_blocks"] and len(set(results["input_batch_blocks"])) > 12


def check_recordable(res):
    """the recorder's own condition: no launching entry point got past its checks"""
    for f in FILES:
        bad = [(i, v) for i, v in enumerate(res[f"refusals_{f}"]) if v > 0]
        if bad:
            sys.exit(f"refusals_{f}: {len(bad)} cases were NOT refused (index, result): {bad[:8]} - a launch was reached with fake pointers; fix the sweep")
        if set(res[f"refusals_{f}"]) != CODES[f]:
            sys.exit(f"refusals_{f}: codes {sorted(set(res[f'refusals_{f}']))}, expected {sorted(CODES[f])}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: [PN2_LIB=<library to record from>] python tests/test_launch_select_tail_cpu.py --record")
    if ENV_SWITCH in os.environ:
        sys.exit("unset PN2_TAIL_BAND: the fixture holds the default geometry")
    from pn2 import capi
    res = sweep(capi)
    check_recordable(res)
    with open(FIXTURE, "w") as f:
        json.dump(res, f, separators=(",", ":"))
        f.write("\n")
    print(f"recorded {sum(len(v) for v in res.values())} results from {capi.LIB_PATH}:")
    for k, v in res.items():
        print(f"  {k:22s} {len(v):6d} results, {len({json.dumps(x) for x in v}):5d} distinct")
