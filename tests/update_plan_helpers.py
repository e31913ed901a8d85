"""The host build of the update plan (scenelib2_amd/csrc/sl2_update_plan.hpp through tests/update_plan_host.cpp) for the tests
that ask it something: tests/test_update_plan_host.py walks a grid through it, tests/test_ekf_update_cases_host.py holds the case
table of the dense update to it."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from scenelib2_amd.monoslam import Engine

HDR = os.path.join(ROOT, "scenelib2_amd", "csrc", "sl2_update_plan.hpp")
SRC = os.path.join(ROOT, "tests", "update_plan_host.cpp")

# one row of up_plans' input and of its output (tests/update_plan_host.cpp)
IN = ("max_features", "n_select", "kpart", "group_from", "panel_from", "B", "build_variant", "chol_variant", "fwd_variant",
      "build_split", "build_ahead", "build_lds_min", "no_ksplit", "fwd_group", "chol_panel", "superseded")
SIZES = ("ld", "ppos", "nsel_max", "mld", "nblk_max", "admitted")
OUT = SIZES + Engine.UPDATE_PLAN_FIELDS + ("error",)

IP = C.POINTER(C.c_int)
_lib = None


def load():
    global _lib
    if _lib is None:
        bdir = os.path.join(ROOT, "tests", "_build")
        os.makedirs(bdir, exist_ok=True)
        so = os.path.join(bdir, "libupdate_plan_host.so")
        if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-shared", "-o", so, SRC])
        L = C.CDLL(so)
        L.up_plans.argtypes = [IP, C.c_int, IP]
        L.up_equal.argtypes = [IP, C.c_int, IP, IP]
        L.up_error_text.restype = C.c_char_p
        assert L.up_in_ints() == len(IN) and L.up_out_ints() == len(OUT)
        _lib = L
    return _lib


def plans_of(inp):
    """inp: int32 [n][len(IN)] -> int64 [n][len(OUT)]."""
    out = np.zeros((len(inp), len(OUT)), dtype=np.int32)
    load().up_plans(inp.ctypes.data_as(IP), len(inp), out.ctypes.data_as(IP))
    return out.astype(np.int64)


def plans_equal(inp, ref):
    """operator== of the plan of every input i against the plan of input ref[i]."""
    ref = np.ascontiguousarray(ref, dtype=np.int32)
    out = np.zeros(len(ref), dtype=np.int32)
    load().up_equal(inp.ctypes.data_as(IP), len(ref), ref.ctypes.data_as(IP), out.ctypes.data_as(IP))
    return out


def plan_of_engine(max_features, n_select, batch, env, superseded):
    """(sizes, plan) of an engine created with these arguments and these switches of the TEST build (SL2_* as sl2_create reads
    them) and one sequence group: the plan as Engine.debug_update_plan gives it, forms by name."""
    frm = int(env["SL2_PANEL_FROM"]) if "SL2_PANEL_FROM" in env else None
    row = dict(max_features=max_features, n_select=n_select, kpart=1, group_from=13 if frm is None else frm,
               panel_from=16 if frm is None else frm, B=batch, build_variant=int(env.get("SL2_BUILD_VARIANT", 1)),
               chol_variant=int(env.get("SL2_CHOL_VARIANT", 1)), fwd_variant=int(env.get("SL2_FWD_VARIANT", 1)),
               build_split=int(env.get("SL2_BUILD_SPLIT", 0)), build_ahead=int(env.get("SL2_BUILD_AHEAD", 1)),
               build_lds_min=int(env.get("SL2_BUILD_LDS_MIN", 0)), no_ksplit=int("SL2_NO_KSPLIT" in env),
               fwd_group=int(env.get("SL2_FWD_GROUP", 8)), chol_panel=int(env.get("SL2_CHOL_PANEL", 8)), superseded=int(superseded))
    assert set(env) <= {"SL2_PANEL_FROM", "SL2_BUILD_VARIANT", "SL2_CHOL_VARIANT", "SL2_FWD_VARIANT", "SL2_BUILD_SPLIT", "SL2_BUILD_AHEAD",
                        "SL2_BUILD_LDS_MIN", "SL2_NO_KSPLIT", "SL2_FWD_GROUP", "SL2_CHOL_PANEL"}, env
    out = dict(zip(OUT, (int(v) for v in plans_of(np.ascontiguousarray([[row[k] for k in IN]], dtype=np.int32))[0])))
    plan = {k: out[k] for k in Engine.UPDATE_PLAN_FIELDS}
    plan.update(build=Engine.BUILD_FORMS[plan["build"]], chol=Engine.CHOL_FORMS[plan["chol"]], fwd=Engine.FWD_FORMS[plan["fwd"]])
    return {k: out[k] for k in SIZES}, plan
