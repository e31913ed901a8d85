"""The frame converter's plan (scenelib2_amd/csrc/sl2_convert_plan.hpp), compiled for the host as a program of its own
(tests/convert_plan_host.cpp, under the address and undefined-behaviour sanitizers; nothing is loaded into Python):
converter_upload takes every sequence's route bits and the plan from it, sl2_convert_frames walks the plan.  Checked here, member
by member, against THE RULES BEFORE THE PLAN, restated from the five places that had to agree by hand: the bits converter_upload
ORed into the device record; its second walk that sorted the sequences into four lists and sized the LDS; the packing of the
lists into one buffer; the offsets sl2_convert_frames re-derived from the lists' sizes; its `listed < nseq` for the linear launch.
The restatement below is written from that code, not from the header."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GRAY8, RGB24, BGR24, UYVY, YUYV = range(5)
GRAY10, GRAY12, GRAY16 = 16, 17, 18
RGGB, GRBG, GBRG, BGGR = 24, 25, 26, 27
DEEP, BAYER = (GRAY10, GRAY12, GRAY16), (RGGB, GRBG, GBRG, BGGR)
FORMATS = (GRAY8, RGB24, BGR24, UYVY, YUYV) + DEEP + BAYER
LINEAR, AREA = 0, 1
# the routes of the header, in its order; the listed ones in the order of the one list buffer
R_NONE, R_LINEAR, R_AREA, R_RAW_LINEAR, R_RAW_AREA, R_REMAP = -1, 0, 1, 2, 3, 4
ROUTE_BITS = {R_NONE: 0, R_LINEAR: 0, R_AREA: 0x100, R_RAW_LINEAR: 0x200, R_RAW_AREA: 0x300, R_REMAP: 0x700}
# the constants, as sl2_convert.hip and sl2_convert_remap.hpp had them
THREADS, BAND_ROWS, SLOTS, LDS_BYTES, RAW_SLOTS, RAW_LDS_BYTES = 256, 8, 16, 4 * (4096 + 16), 18, 4 * (4096 + 16)
AREA_BIT, RAW_BIT, REMAP_BIT, FORMAT_MASK = 0x100, 0x200, 0x400, 0xff


def pad(w):
    """A staged row: (W + 15 + 15) & ~15, as the kernels and converter_upload wrote it."""
    return (w + 15 + 15) & ~15


def seq(fmt, flt=LINEAR, width=64, slot=-1, have=1):
    return (have, width, fmt, flt, slot)


UNSET = (0, 0, 0, LINEAR, -1)


# ------------------------------------------------------------------------------------ the rules before the plan, restated
def rules_before_the_plan(out_h, seqs):
    is_raw = lambda fmt: fmt in DEEP or fmt in BAYER
    # converter_upload, first walk: the device record's format word (only of sequences with a source)
    bits = []
    for have, width, fmt, flt, slot in seqs:
        b = 0
        if flt == AREA:
            b |= 0x100
        if is_raw(fmt):
            b |= 0x200
        if slot >= 0:
            b |= 0x400 | 0x100 | 0x200
        bits.append(b if have else None)
    # converter_upload, second walk: the four lists and the sizes
    area, raw_linear, raw_area, remap_list = [], [], [], []
    widest = raw_widest = raw_linear_stage = raw_area_stage = 0
    for s, (have, width, fmt, flt, slot) in enumerate(seqs):
        if not have:
            continue
        if slot >= 0:
            remap_list.append(s)
            continue
        if not is_raw(fmt):
            if flt == AREA:
                area.append(s)
                widest = max(widest, width)
            continue
        (raw_area if flt == AREA else raw_linear).append(s)
        if flt == AREA:
            raw_widest = max(raw_widest, width)
        if fmt in BAYER:
            want = 18 * ((width + 15 + 15) & ~15)
            if flt == AREA:
                raw_area_stage = max(raw_area_stage, min(want, RAW_LDS_BYTES))
            else:
                raw_linear_stage = max(raw_linear_stage, min(want, RAW_LDS_BYTES))
    area_lds = 4 * ((widest + 3) // 4 * 4)
    raw_area_colsum = 4 * ((raw_widest + 3) // 4 * 4)
    lists = area + raw_linear + raw_area + remap_list
    # sl2_convert_frames: the offsets it re-derived, its launches and their dynamic LDS
    listed = len(area) + len(raw_linear) + len(raw_area) + len(remap_list)
    nhave = sum(1 for q in seqs if q[0])
    return dict(
        bits=bits, lists=lists, bands=(out_h + 8 - 1) // 8,
        linear_launch=listed < len(seqs) if nhave == len(seqs) else None,          # the call refuses a converter with an unset sequence
        count=[nhave - listed, len(area), len(raw_linear), len(raw_area), len(remap_list)],
        start=[0, 0, len(area), len(area) + len(raw_linear), len(area) + len(raw_linear) + len(raw_area)],
        lds=[0, area_lds, raw_linear_stage, raw_area_colsum + raw_area_stage, 0],
        colsum=raw_area_colsum, raw_area_stage=raw_area_stage)


# ------------------------------------------------------------------------------------------------------------------ the grid
def bayer_widths_at_the_cap():
    """The widest Bayer source whose eighteen padded rows fit kRawLdsBytes, and the next one: from the rule."""
    fits = [w for w in range(2, 4097) if 18 * pad(w) <= RAW_LDS_BYTES]
    return max(fits), max(fits) + 1


def _cases():
    cases = []
    add = lambda out_h, seqs: cases.append((out_h, list(seqs)))
    every = [seq(fmt, flt, 40 + 8 * i, slot) for i, (fmt, flt, slot) in
             enumerate((fmt, flt, slot) for fmt in FORMATS for flt in (LINEAR, AREA) for slot in (-1, 0, 3))]
    # nseq of 1: every format, filter, mapped or not
    for q in every:
        add(48, [q])
    # all of them in one batch, then with sequences without a source between them, at the front and at the end
    add(240, every)
    gaps = [UNSET]
    for i, q in enumerate(every):
        gaps.append(q)
        if i % 3 == 0:
            gaps.append(UNSET)
        if i % 7 == 0:
            gaps.append(seq(RGGB, AREA, 4096, 2, have=0))      # what an unset record holds does not count
    add(9, gaps)
    add(1, [UNSET])
    add(8, [UNSET, UNSET, seq(GRAY12, AREA, 33), UNSET])
    # a batch that is all one route, for each of the five
    one = {R_LINEAR: seq(YUYV), R_AREA: seq(RGB24, AREA, 640), R_RAW_LINEAR: seq(GRBG, LINEAR, 640), R_RAW_AREA: seq(GRAY10, AREA, 640),
           R_REMAP: seq(BGGR, AREA, 640, 1)}
    for r in one:
        add(48, [one[r]] * 4)
    # every subset of the four listed routes, with and without linear sequences, at different counts and interleaved: an empty route
    # after a non-empty one has a start where its count is zero
    for mask in range(16):
        for with_linear in (0, 1):
            routes = [r for k, r in enumerate((R_AREA, R_RAW_LINEAR, R_RAW_AREA, R_REMAP)) if mask >> k & 1] + [R_LINEAR] * with_linear
            if not routes:
                continue
            counts = {r: 1 + (r + mask) % 4 for r in routes}
            batch = []
            while any(counts.values()):
                for r in routes:
                    if counts[r]:
                        counts[r] -= 1
                        batch.append(one[r])
            add(48, batch)
    add(48, [one[R_AREA]] * 1 + [one[R_RAW_LINEAR]] * 2 + [one[R_LINEAR]] * 5 + [one[R_RAW_AREA]] * 3 + [one[R_REMAP]] * 4)
    # the raw stage: Bayer widths either side of the cap, 2 and 4096, in either raw route alone (the other's stage stays 0 although
    # it lists deep grey sources, wider ones too), and the widest Bayer source not the first listed
    fit, capped = bayer_widths_at_the_cap()
    for w in (2, fit, capped, 4096):
        for fmt in BAYER[:2]:
            add(48, [seq(fmt, LINEAR, w), seq(GRAY16, AREA, 4096), seq(GRAY12, LINEAR, 4096)])
            add(48, [seq(fmt, AREA, w), seq(GRAY16, AREA, 4000), seq(GRAY12, LINEAR, 4096)])
    add(48, [seq(RGGB, LINEAR, 100), seq(BGGR, LINEAR, fit), seq(GBRG, LINEAR, 320), seq(GRBG, AREA, 2), seq(RGGB, AREA, 640), seq(GRBG, AREA, 16)])
    add(48, [seq(RGGB, LINEAR, capped, 0), seq(BGGR, AREA, 4096, 1), seq(GBRG, LINEAR, 320), seq(GRBG, AREA, 322)])      # mapped Bayer sources size nothing
    # colsum: widths 1, 4, 5 and 4096, alone and with the widest source not the first listed, in both area routes
    for widths in ((1,), (4,), (5,), (4096,), (4, 5, 1), (1, 4096, 4), (5, 4), (1, 1, 4)):
        add(48, [seq(GRAY8, AREA, w) for w in widths])
        add(48, [seq(GRAY16, AREA, w) for w in widths])
        add(48, [seq(UYVY, AREA, w) for w in widths] + [seq(GRAY10, AREA, w) for w in reversed(widths)] + [seq(RGB24, LINEAR, 4096)])
    # bands
    for out_h in (1, 7, 8, 9, 16, 17, 4095, 4096):
        add(out_h, [one[R_LINEAR], one[R_RAW_AREA]])
    # and batches drawn at random
    rng = np.random.default_rng(20240)
    for _ in range(300):
        n = int(rng.integers(1, 13))
        add(int(rng.integers(1, 4097)),
            [seq(int(rng.choice(FORMATS)), int(rng.integers(0, 2)), int(rng.choice((1, 2, 4, 5, 640, fit, capped, 1920, 4096))),
                 int(rng.choice((-1, -1, 0, 5))), int(rng.integers(0, 5) != 0)) for _ in range(n)])
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    """tests/convert_plan_host.cpp built with the sanitizers and run once over CASES: (constants, route bits, a dict per case)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    tmp = str(tmp_path_factory.mktemp("convert_plan"))
    exe = os.path.join(tmp, "convert_plan_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                           os.path.join(ROOT, "tests", "convert_plan_host.cpp")])
    path = os.path.join(tmp, "cases.txt")
    with open(path, "w") as f:
        f.write("%d\n" % len(CASES))
        for out_h, seqs in CASES:
            f.write("%d %d\n" % (len(seqs), out_h))
            f.writelines("%d %d %d %d %d\n" % q for q in seqs)
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr
    lines = res.stdout.splitlines()
    assert lines[-1] == "ok %d cases" % len(CASES)
    ints = lambda line, name: [int(v) for v in line.split()[1:]] if line.split()[0] == name else pytest.fail(line)
    constants, route_bits = ints(lines[0], "constants"), ints(lines[1], "route_bits")
    names = ("count", "start", "lds", "colsum", "bands", "route", "bits", "list")
    plans = []
    for k in range(len(CASES)):
        block = lines[2 + k * (1 + len(names)):2 + (k + 1) * (1 + len(names))]
        assert block[0] == "case %d" % k
        plans.append({name: ints(line, name) for name, line in zip(names, block[1:])})
    return constants, route_bits, plans


def test_the_grid_holds_what_it_is_meant_to():
    rules = [rules_before_the_plan(out_h, seqs) for out_h, seqs in CASES]
    single = {q[1:] for _, seqs in CASES if len(seqs) == 1 for q in seqs if q[0]}
    assert {(fmt, flt, slot >= 0) for _, fmt, flt, slot in single} == {(fmt, flt, m) for fmt in FORMATS for flt in (LINEAR, AREA) for m in (False, True)}
    assert len(FORMATS) == 12
    # a mapped Bayer sequence with AREA is on the remap list only
    assert any(len(seqs) == 1 and seqs[0][2] in BAYER and seqs[0][3] == AREA and seqs[0][4] >= 0 and r["count"] == [0, 0, 0, 0, 1]
               and r["lds"] == [0] * 5 and r["bits"] == [0x700] for (_, seqs), r in zip(CASES, rules))
    # sequences without a source between sequences that have one
    assert any(any(not a[0] and b[0] for a, b in zip(seqs, seqs[1:])) and any(a[0] and not b[0] for a, b in zip(seqs, seqs[1:])) for _, seqs in CASES)
    # all one route, each of the five; all four listed routes at different counts; an empty route after a non-empty one
    for r in range(5):
        assert any(c["count"][r] == sum(c["count"]) >= 2 for c in rules), r
    assert any(len(set(c["count"][1:])) == 4 and min(c["count"]) > 0 for c in rules)
    for r in (2, 3, 4):
        assert any(c["count"][r] == 0 and c["count"][r - 1] > 0 and c["start"][r] > 0 for c in rules), r
    # the raw stage: the two widths from the rule, the cap met on either side, one route's stage 0 beside the other's
    fit, capped = bayer_widths_at_the_cap()
    assert (fit, capped) == (897, 898) and 18 * pad(fit) == 16416 <= RAW_LDS_BYTES == 16448 < 18 * pad(capped) == 16704
    stages = {(c["lds"][2], c["raw_area_stage"]) for c in rules}
    for w in (2, fit, capped, 4096):
        want = min(18 * pad(w), RAW_LDS_BYTES)
        assert (want, 0) in stages and (0, want) in stages, w
    assert any(c["lds"][2] == 0 and c["count"][2] > 0 and c["raw_area_stage"] > 0 for c in rules)
    assert any(c["raw_area_stage"] == 0 and c["count"][3] > 0 and c["lds"][2] > 0 for c in rules)
    # colsum: 1, 4, 5 and 4096 columns, the widest not the first listed
    for r in (1, 3):
        widest = {max(seqs[s][1] for s in c["lists"][c["start"][r]:c["start"][r] + c["count"][r]]) for (_, seqs), c in zip(CASES, rules) if c["count"][r]}
        assert {1, 4, 5, 4096} <= widest, r
    assert {16, 32, 16384} <= {c["lds"][1] for c in rules} and {16, 32, 16384} <= {c["colsum"] for c in rules}
    assert any(seqs[c["lists"][0]][1] < max(seqs[s][1] for s in c["lists"][:c["count"][1]]) for (_, seqs), c in zip(CASES, rules) if c["count"][1] > 1)
    assert {1, 2, 512} <= {c["bands"] for c in rules}


def test_constants_and_route_bits_are_what_the_two_units_had(program_output):
    constants, route_bits, _ = program_output
    assert constants == [THREADS, BAND_ROWS, SLOTS, LDS_BYTES, RAW_SLOTS, RAW_LDS_BYTES, AREA_BIT, RAW_BIT, REMAP_BIT, FORMAT_MASK,
                         pad(1), pad(2), pad(3), pad(4096)]
    assert (pad(1), pad(2), pad(3), pad(4096)) == (16, 32, 32, 4112)
    assert route_bits == [0, 0, 0x100, 0x200, 0x300, 0x700] == [ROUTE_BITS[r] for r in range(-1, 5)]


def test_the_plan_equals_the_rules_before_the_plan_on_every_case(program_output):
    _, _, plans = program_output
    assert len(plans) == len(CASES)
    for k, ((out_h, seqs), got) in enumerate(zip(CASES, plans)):
        want = rules_before_the_plan(out_h, seqs)
        where = (k, out_h, seqs)
        assert got["count"] == want["count"], where
        assert got["list"] == want["lists"], where
        assert got["bands"] == [want["bands"]], where
        # a start counts where its route has a sequence, and also where it has none (sl2_convert_frames derived all of them)
        assert got["start"][1:] == want["start"][1:] and got["start"][0] == 0, where
        for r in range(1, 5):
            assert got["list"][got["start"][r]:got["start"][r] + got["count"][r]] == [s for s in want["lists"] if got["route"][s] == r], where
        assert got["lds"] == want["lds"] and got["colsum"] == [want["colsum"]], where
        assert got["lds"][3] - got["colsum"][0] == want["raw_area_stage"], where          # k_raw_area's third argument
        if want["linear_launch"] is not None:
            assert (got["count"][0] > 0) == want["linear_launch"], where
        for s, q in enumerate(seqs):
            if q[0]:
                assert got["bits"][s] == want["bits"][s] == ROUTE_BITS[got["route"][s]], (where, s)
                assert (got["route"][s] == R_LINEAR) == (s not in want["lists"]), (where, s)
            else:
                assert got["route"][s] == R_NONE and got["bits"][s] == 0 and s not in got["list"], (where, s)
