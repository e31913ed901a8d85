"""The step plan (scenelib2_amd/csrc/sl2_step_plan.hpp), compiled for the host: sl2_go_one_step makes one plan per step, issues
its launches from it and keys captured steps (HIP graphs) by it.  Checked here over every input of a grid, against the rules
restated from the code before the plan existed (three places that had to agree by hand: the graph key's hash, the launch list
of sl2_go_one_step, and the launchers' own conditions):
  - the plan says what those rules say;
  - the plan is never a finer key than the old one (equal old keys -> equal plans; it may be coarser);
  - the plan is a sufficient key (equal plans -> the same launches with the same baked arguments)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "scenelib2_amd", "csrc", "sl2_step_plan.hpp")
SRC = os.path.join(ROOT, "tests", "step_plan_host.cpp")

SHAPES = [(16, 128, 32, 1), (128, 448, 32, 1), (100, 384, 256, 4)]         # (N, ld, mld, kpart)
BATCHES = [(1, 1), (256, 1), (257, 1), (1024, 1), (1024, 3)]               # (sequences, groups)
SMALL_M, SMALL_W, SMALL_BATCH_MAX = 32, 128, 256


def group_counts(B, G):
    """sl2_seq_arrays.hpp: group_range - B / G each, the first B % G groups one longer."""
    return [B // G + (1 if k < B % G else 0) for k in range(G)]


# ---------------------------------------------------------------- the rules of the code before the plan, restated

def old_mode(inp, Bg):
    N, ld, mld, kpart, fusion, used, Bl, Bs, sb, ps, st, em = inp
    if not fusion or mld != SMALL_M or kpart != 1 or 13 + 3 * sb + 6 * kpart + 1 > SMALL_W:
        return 0
    return 1 if (Bg <= SMALL_BATCH_MAX or ld >= 256 or fusion == 2) else 2


def old_panel(inp):
    kpart, sb = inp[3], inp[8]
    return 64 if 13 + 3 * sb + 6 * kpart + 1 <= 64 else SMALL_W


def old_key(inp, counts):
    """(save_trajectory, enable_mapping, tail, small_any) of a captured step, small_any as sl2_go_one_step hashed it."""
    N, ld, mld, kpart, fusion, used, Bl, Bs, sb, ps, st, em = inp
    tail = 1 if used else 0
    parts = ps if tail else 0
    m = (1 if sb + 1 > N else 0) + 2 * parts
    for Bg in counts:
        md = old_mode(inp, Bg)
        m = (m * 7 + (0 if md == 0 else md + (3 if old_panel(inp) == 64 else 0))) % 1000003
    return (st, em, tail, m)


def old_launches(inp):
    """What the step launched, with the per-step choices its launches carried as arguments: per group size (a longer group, a
    shorter one) and for the feature-initialisation tail.  (How many groups there are is the engine's, not the step's.)"""
    N, ld, mld, kpart, fusion, used, Bl, Bs, sb, ps, st, em = inp
    tail = bool(used)
    out = []
    for Bg in (Bl, Bs):
        mode = old_mode(inp, Bg)
        st_g = 0 if tail else st
        front = ["k_small_front"] if mode == 1 else ["k_predict", "k_feature_prediction", "k_select"]
        if mode:
            back = ["search", ("k_small_back", "lds panel", old_panel(inp), "save_trajectory", st_g)]
        else:
            back = ["search", "k_search_score", "update", ("k_finalize", "save_trajectory", st_g)]
        out.append(tuple(front + back))
    t = []
    if tail:
        none, full = ps == 1, ps == 2
        t.append(("MapParams", 1 if em else 0, st, "parts_skipped", 1 if none else 0))
        if em and sb + 1 > N:
            t.append("k_map_compact_slots")
        if not full:
            t.append("k_map_find")
        if none:
            t.append("k_map_finish")
        else:
            if not full:
                t.append("k_map_create")
            t += [("k_map_particles", "parts_full", 1 if full else 0), "k_map_me_search", "k_me_big", "k_map_update"]
    out.append(tuple(t))
    return tuple(out)


def expected_plan(inp):
    """The 17 members of the plan (tests/step_plan_host.cpp: sp_plans), from the rules above."""
    N, ld, mld, kpart, fusion, used, Bl, Bs, sb, ps, st, em = inp
    row = []
    for Bg in (Bl, Bs):
        mode = old_mode(inp, Bg)
        row += [int(mode == 1), int(mode != 0), old_panel(inp) if mode else 0, 0 if used else st]
    if not used:
        return row + [0] * 9
    return row + [1, 1 if em else 0, st, int(bool(em) and sb + 1 > N), int(ps != 2), int(ps == 0), int(ps != 1), int(ps == 1), int(ps == 2)]


def walk(plan):
    """The launches of a plan, the way sl2_go_one_step and launch_mapping walk it."""
    out = []
    for k in range(2):
        small_front, small_back, panel_w, st_g = plan[4 * k:4 * k + 4]
        front = ["k_small_front"] if small_front else ["k_predict", "k_feature_prediction", "k_select"]
        if small_back:
            back = ["search", ("k_small_back", "lds panel", panel_w, "save_trajectory", st_g)]
        else:
            back = ["search", "k_search_score", "update", ("k_finalize", "save_trajectory", st_g)]
        out.append(tuple(front + back))
    runs, em, st, squeeze, find, create, partials, finish, parts_full = plan[8:]
    t = []
    if runs:
        t.append(("MapParams", em, st, "parts_skipped", 1 if finish else 0))
        t += ["k_map_compact_slots"] * squeeze + ["k_map_find"] * find + ["k_map_finish"] * finish + ["k_map_create"] * create
        if partials:
            t += [("k_map_particles", "parts_full", parts_full), "k_map_me_search", "k_me_big", "k_map_update"]
    out.append(tuple(t))
    return tuple(out)


# ---------------------------------------------------------------- the grid

@pytest.fixture(scope="module")
def sp():
    bdir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libstep_plan_host.so")
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    ip = C.POINTER(C.c_int)
    L.sp_plans.argtypes = [ip, C.c_int, ip]
    L.sp_equal.argtypes = [ip, C.c_int, ip, ip]
    return L


@pytest.fixture(scope="module")
def grid(sp):
    """Every input of the grid, the groups' sequence counts of each, and the plans the header makes of them."""
    assert sp.sp_in_ints() == 12 and sp.sp_out_ints() == 17
    inputs, counts = [], []
    for (N, ld, mld, kpart), (B, G) in itertools.product(SHAPES, BATCHES):
        c = group_counts(B, G)
        assert len(set(c)) <= 2 and c == sorted(c, reverse=True)
        for fusion, used, sb, ps, st, em in itertools.product((0, 1, 2), (0, 1), range(N + 2), (0, 1, 2), (0, 1), (0, 1)):
            inputs.append((N, ld, mld, kpart, fusion, used, c[0], c[-1], sb, ps, st, em))
            counts.append(c)
    arr = np.ascontiguousarray(inputs, dtype=np.int32)
    plans = np.zeros((len(inputs), 17), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    sp.sp_plans(arr.ctypes.data_as(ip), len(inputs), plans.ctypes.data_as(ip))
    return inputs, counts, arr, [tuple(int(v) for v in row) for row in plans]


def plans_equal(sp, arr, ref):
    """operator== of the plan of every input i against the plan of input ref[i]."""
    ip = C.POINTER(C.c_int)
    ref = np.ascontiguousarray(ref, dtype=np.int32)
    out = np.zeros(len(ref), dtype=np.int32)
    sp.sp_equal(arr.ctypes.data_as(ip), len(ref), ref.ctypes.data_as(ip), out.ctypes.data_as(ip))
    return out


def test_header_needs_no_hip():
    text = open(HDR).read()
    assert "hip_runtime" not in text and "#include" not in text


def test_constants(sp):
    assert [sp.sp_constant(k) for k in range(3)] == [SMALL_M, SMALL_W, SMALL_BATCH_MAX]


def test_plan_is_what_the_rules_say(grid):
    inputs, _, _, plans = grid
    assert len(inputs) == 5 * 72 * (18 + 130 + 102)
    for inp, plan in zip(inputs, plans):
        assert list(plan) == expected_plan(inp), inp
        assert walk(plan) == old_launches(inp), inp
    # every kind of step the grid is there for was reached
    seen = {(p[0], p[1], p[2]) for p in plans} | {(p[4], p[5], p[6]) for p in plans}
    assert seen == {(0, 0, 0), (1, 1, 64), (1, 1, 128), (0, 1, 64), (0, 1, 128)}
    assert {p[8:] for p in plans if p[8]} >= {(1, 1, 1, 1, 1, 1, 1, 0, 0), (1, 0, 0, 0, 1, 0, 0, 1, 0), (1, 1, 1, 0, 0, 0, 1, 0, 1)}
    assert all(p[:4] == p[4:8] for p in plans)                # no batch of the grid has groups on both sides of the 256 rule ...


def test_groups_of_two_sizes_get_a_plan_each(sp):
    """... so here is one that has: 513 sequences in two groups, 257 + 256, at a small capacity."""
    c = group_counts(513, 2)
    assert c == [257, 256]
    arr = np.ascontiguousarray([(16, 128, 32, 1, 1, 0, c[0], c[1], 12, 0, 1, 0)], dtype=np.int32)
    out = np.zeros((1, 17), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    sp.sp_plans(arr.ctypes.data_as(ip), 1, out.ctypes.data_as(ip))
    assert list(out[0][:8]) == [0, 1, 64, 1, 1, 1, 64, 1]


def test_the_plan_is_never_a_finer_key_than_the_old_one(sp, grid):
    inputs, counts, arr, plans = grid
    first = {}
    ref = [first.setdefault(old_key(inp, c), i) for i, (inp, c) in enumerate(zip(inputs, counts))]
    assert plans_equal(sp, arr, ref).all()
    assert all(plans[i] == plans[r] for i, r in enumerate(ref))
    # and it is coarser where the old key held a bit no launch depended on: the squeeze bit with mapping off
    assert len(set(plans)) < len(first)


def test_equal_plans_launch_the_same_with_the_same_arguments(sp, grid):
    inputs, _, arr, plans = grid
    first = {}
    ref = [first.setdefault(p, i) for i, p in enumerate(plans)]
    assert plans_equal(sp, arr, ref).all()
    for i, r in enumerate(ref):
        assert old_launches(inputs[i]) == old_launches(inputs[r]), (inputs[i], inputs[r])
    # operator== looks at every member: any two plans that differ anywhere are unequal
    reps = sorted(first.values())
    pairs = [(a, b) for a in reps for b in reps if a != b]
    sub = np.ascontiguousarray(arr[[a for a, _ in pairs]])
    other = np.ascontiguousarray(arr[[b for _, b in pairs]])
    both = np.ascontiguousarray(np.concatenate([sub, other]))
    assert not plans_equal(sp, both, list(range(len(pairs), 2 * len(pairs))))[:len(pairs)].any()
