"""The update plan (scenelib2_amd/csrc/sl2_update_plan.hpp), compiled for the host: sl2_create takes the sizes of the innovation
system from update_sizes, launch_update makes one plan per call and walks it.  Checked here, member by member, over every input
of a grid that straddles every edge, against THE RULES BEFORE THE PLAN, restated from the five places that had to agree by hand
(sl2_create; launch_update_range; launch_fwdsub_lds; launch_chol_panels and launch_fwdsub_grouped; a Python copy in
tests/ekf_update_cases.py, which is where this restatement comes from, completed with the ahead rule, the threads and the LDS
bytes).  One deliberate difference: where launch_fwdsub_lds fell through its switch without a launch (TEST build, SL2_PANEL_FROM
above 13 and 14 or more blocks) the plan says grouped, re-read or none.

Members a form has no use for are zero in the plan (threads aside, the two-pass build has no nsplit or LDS; only panels have a
panel width, only the one-launch substitution an instantiation, only the grouped one a group), so that equal plans mean equal
launches and nothing else."""
import itertools

import numpy as np
import pytest

import update_plan_helpers as uh
from update_plan_helpers import IN, OUT

# the constants, as the kernels' sources had them (tests/update_plan_host.cpp: up_constant, in this order)
AS_BATCH, AHEAD_ENTRY, AHEAD_LDS_MAX, ONE_THREAD_LD, FULL_BATCH, WORKGROUPS = 4, 24, 40960, 1024, 1024, 3072
KS_MAX_BLOCKS, KS_MAX_STRIPS, LDS_MAX_BLOCKS, PANEL_BLOCKS, LD_MAX, MLD_MAX = 8, 160, 13, 4, 2048, 1024
CONSTANTS = [AS_BATCH, AHEAD_ENTRY, AHEAD_LDS_MAX, ONE_THREAD_LD, FULL_BATCH, WORKGROUPS, KS_MAX_BLOCKS, KS_MAX_STRIPS,
             LDS_MAX_BLOCKS, PANEL_BLOCKS, LD_MAX, MLD_MAX]

# the enums of the header
TWO_PASS, AS14, AS22, AHEAD4, AHEAD2 = range(5)
CHOL_NONE, LEFT, PANELS, PER_BLOCK = range(4)
FWD_NONE, KSPLIT, LDS, GROUPED, REREAD = range(5)
SKIPPED = -1          # the rules before the plan only: launch_fwdsub_lds' `default: break`

ERR_CHOL = "launch_update: no factorisation for this system size (sl2_create should have padded it)"
ERR_FWD = "launch_update: no substitution kernel for this system size (sl2_create should have padded it)"

# ------------------------------------------------------------------------------------------------------------------ the grid
MAX_FEATURES = [5, 6, 7, 8, 24, 64, 100, 122, 142, 143, 334, 335, 676, 677]
N_SELECT = [1, 16, 17, 42, 43, 64, 65, 128, 129, 208, 209, 256, 257, 512, 513]
BATCHES = [1, 2, 20, 21, 1023, 1024, 3072, 3073]
FROM = [(13, 16), (2, 2), (14, 14)]                     # (group_from, panel_from): the default; SL2_PANEL_FROM = 2, 14 sets both
KNOBS = list(itertools.product(
    FROM, (0, 1), (0, 1), (0, 1),                       # build_variant, chol_variant, fwd_variant
    (0, 1, 3), (0, 1), (0, 65536), (0, 1),              # build_split, build_ahead, build_lds_min, no_ksplit
    (4, 8), (4, 8), (0, 1)))                            # fwd_group, chol_panel, superseded


def ld_of(max_features, kpart=1):
    return (13 + 3 * max_features + 6 * kpart + 1 + 63) // 64 * 64


def batches_of(max_features):
    """The grid's batches, and for this ld the two on either side of 160 strips."""
    b0 = KS_MAX_STRIPS // (ld_of(max_features) // 16)
    return sorted(set(BATCHES) | {b0, b0 + 1})


_KNOB_ROWS = np.array([(gf, pf, 0, bv, cv, fv, split, ahead, lds_min, noks, fg, cp, sup)
                       for (gf, pf), bv, cv, fv, split, ahead, lds_min, noks, fg, cp, sup in KNOBS], dtype=np.int32)


def inputs_of(max_features, n_select):
    """Every input of the grid with these two sizes: batches x knobs, one row of IN each."""
    bs = batches_of(max_features)
    rows = np.tile(_KNOB_ROWS, (len(bs), 1))
    rows[:, 2] = np.repeat(np.array(bs, dtype=np.int32), len(_KNOB_ROWS))
    head = np.empty((len(rows), 3), dtype=np.int32)
    head[:] = (max_features, n_select, 1)
    return np.ascontiguousarray(np.concatenate([head, rows], axis=1))


# ------------------------------------------------------------------------------------ the rules before the plan, restated
def up(a, b):
    return (a + b - 1) // b * b


def rules_before_the_plan(inp):
    """inp: [n][len(IN)].  Every member of OUT as the code before the plan computed or implied it, as arrays over the inputs;
    fwd is SKIPPED where launch_fwdsub_lds fell through."""
    i = {k: inp[:, j].astype(np.int64) for j, k in enumerate(IN)}
    mf, B, sup = i["max_features"], i["B"], i["superseded"] != 0
    # sl2_create
    ld = up(13 + 3 * mf + 6 * i["kpart"] + 1, 64)
    nsel = np.minimum(np.maximum(i["n_select"], 1), mf)
    mld = up(2 * nsel, 32)
    mld = np.where(mld // 32 > i["group_from"], up(2 * nsel, 64), mld)
    mld = np.where(mld // 32 > i["panel_from"], up(2 * nsel, 128), mld)
    nblk = mld // 32
    admitted = ~((ld > 2048) | (mld > 1024))
    # launch_update_range: k_build_A + k_build_S | k_build_AS<1,4> | <2,2> | k_build_AS_ahead<4> | <2>
    two_pass = sup & (i["build_variant"] == 0)
    nsplit = np.where(B >= 1024, 1, (3072 + B - 1) // B)
    nsplit = np.where(i["build_split"] > 0, i["build_split"], nsplit)
    nsplit = np.minimum(np.maximum(nsplit, 1), (mf + 4 - 1) // 4)
    may_ahead = (nsplit == 1) & (ld <= 1024) & (i["build_ahead"] != 0)
    tab = 8 * 24 * nsel
    ahead = np.where(may_ahead & (8 * 2 * 4 * ld + tab <= 40960), 4, np.where(may_ahead & (8 * 2 * 2 * ld + tab <= 40960), 2, 0))
    build = np.where(ahead == 4, AHEAD4, np.where(ahead == 2, AHEAD2, np.where(ld <= 1024, AS14, AS22)))
    threads = np.where(build == AS22, 1024, ld)
    lds = np.where(ahead > 0, 8 * (2 * ahead * ld + 24 * nsel), np.where(ld <= 1024, 8 * 2 * 4 * ld, 8 * 2 * 2 * ld))
    lds = np.where(build != AS22, np.maximum(lds, i["build_lds_min"]), lds)
    build = np.where(two_pass, TWO_PASS, build)
    threads = np.where(two_pass, np.minimum(ld, 512), threads)
    nsplit = np.where(two_pass, 1, nsplit)
    lds = np.where(two_pass, 0, lds)
    # launch_update_range: panels | k_chol_left | the three launches per block column (TEST build) or the refusal
    cv = i["chol_variant"]
    panels = (nblk > i["panel_from"]) & (cv >= 1) & (mld % 64 == 0) & (nblk % 4 == 0)
    left = ~panels & (nblk <= i["panel_from"]) & (cv == 1)
    chol = np.where(panels, PANELS, np.where(left, LEFT, np.where(sup, PER_BLOCK, CHOL_NONE)))
    panel_blocks = np.where(panels, np.where(i["chol_panel"] == 8, 8, 4), 0)      # launch_chol_panels
    # launch_fwdsub_lds, then launch_update_range
    fv1 = i["fwd_variant"] == 1
    ksplit = fv1 & (nblk <= 8) & (B * (ld // 16) <= 160) & (i["no_ksplit"] == 0)
    beyond = fv1 & ~ksplit & (nblk > i["group_from"])
    one_launch = fv1 & ~ksplit & ~beyond
    grouped = beyond & (mld % 64 == 0)
    fwd = np.where(ksplit, KSPLIT, np.where(one_launch, np.where(nblk <= 13, LDS, SKIPPED),
                                            np.where(grouped, GROUPED, np.where(sup, REREAD, FWD_NONE))))
    fwd_nb = np.where(fwd == LDS, nblk, 0)
    group_rows = np.where(fwd == GROUPED, np.where(i["fwd_group"] == 4, 4, 8), 0)     # launch_fwdsub_grouped
    error = np.where(chol == CHOL_NONE, 1, np.where(fwd == FWD_NONE, 2, 0))
    cols = dict(ld=ld, ppos=13 + 3 * mf, nsel_max=nsel, mld=mld, nblk_max=nblk, admitted=admitted, build=build,
                build_threads=threads, build_nsplit=nsplit, build_lds_bytes=lds, chol=chol, chol_panel_blocks=panel_blocks, fwd=fwd,
                fwd_nb=fwd_nb, fwd_group_rows=group_rows, error=error)
    return np.stack([cols[k].astype(np.int64) for k in OUT], axis=1)


def with_the_one_deliberate_change(inp, want):
    """Where the old code launched no substitution at all: grouped on 64-row tiles, else the re-read kernel (TEST build) or the
    refusal.  Returns the rows the change applies to."""
    want = want.copy()
    f, e = OUT.index("fwd"), OUT.index("error")
    skipped = want[:, f] == SKIPPED
    sup = inp[:, IN.index("superseded")] != 0
    tiles = want[:, OUT.index("mld")] % 64 == 0
    want[:, f] = np.where(skipped, np.where(tiles, GROUPED, np.where(sup, REREAD, FWD_NONE)), want[:, f])
    want[:, OUT.index("fwd_group_rows")] = np.where(skipped & tiles, np.where(inp[:, IN.index("fwd_group")] == 4, 4, 8),
                                                    want[:, OUT.index("fwd_group_rows")])
    want[:, e] = np.where(skipped & (want[:, e] == 0) & (want[:, f] == FWD_NONE), 2, want[:, e])
    return want, skipped


# ------------------------------------------------------------------------------------------------------- the compiled plan
@pytest.fixture(scope="module")
def lib():
    return uh.load()


class Grid:
    """The grid in chunks of one (max_features, n_select) each - (inputs, what the header makes of them) -, made when asked for:
    nine million rows are walked, not kept."""

    def __init__(self):
        self._compared = None

    def chunks(self, max_features=None, n_select=None):
        for mf, ns in itertools.product(MAX_FEATURES, N_SELECT):
            if max_features in (None, mf) and n_select in (None, ns):
                inp = inputs_of(mf, ns)
                yield inp, uh.plans_of(inp)

    def compared(self):
        """One walk against the rules before the plan: rows in all, the first that differs, and the rows of the one change."""
        if self._compared is None:
            total, bad, changed = 0, None, []
            for inp, got in self.chunks():
                want, skipped = with_the_one_deliberate_change(inp, rules_before_the_plan(inp))
                total += len(inp)
                differs = np.nonzero((got != want).any(axis=1))[0]
                if differs.size and bad is None:
                    r = differs[0]
                    bad = (dict(zip(IN, inp[r])), dict(zip(OUT, got[r])), dict(zip(OUT, want[r])))
                changed.append((inp[skipped], got[skipped]))
            self._compared = dict(total=total, bad=bad, changed_in=np.concatenate([c[0] for c in changed]),
                                  changed_out=np.concatenate([c[1] for c in changed]))
        return self._compared


@pytest.fixture(scope="module")
def grid():
    return Grid()


def test_header_needs_no_hip():
    text = open(uh.HDR).read()
    assert "hip_runtime" not in text and "#include" not in text


def test_constants_and_texts(lib):
    assert [lib.up_constant(k) for k in range(len(CONSTANTS) + 1)] == CONSTANTS + [-1]
    assert lib.up_error_text(0) is None
    assert lib.up_error_text(1).decode() == ERR_CHOL and lib.up_error_text(2).decode() == ERR_FWD


def test_plan_is_what_the_rules_before_it_say(grid):
    c = grid.compared()
    assert c["bad"] is None, c["bad"]
    assert c["total"] == len(N_SELECT) * len(KNOBS) * sum(len(batches_of(mf)) for mf in MAX_FEATURES)
    print("update-plan grid: %d inputs" % c["total"])


def rows(grid, **eq):
    """(input, plan) of every row of the grid whose named inputs / outputs have the given values."""
    for inp, got in grid.chunks(eq.get("max_features"), eq.get("n_select")):
        m = np.ones(len(inp), dtype=bool)
        for k, v in eq.items():
            m &= (inp[:, IN.index(k)] if k in IN else got[:, OUT.index(k)]) == v
        for r in np.nonzero(m)[0]:
            yield dict(zip(IN, inp[r])), dict(zip(OUT, got[r]))


PRODUCT = dict(superseded=0, build_variant=1, chol_variant=1, fwd_variant=1, group_from=13, panel_from=16, build_split=0,
               build_ahead=1, build_lds_min=0, no_ksplit=0, fwd_group=8, chol_panel=8)


def test_grid_contains_the_named_edges(grid):
    def forms(what, **eq):
        return {p[what] for _, p in rows(grid, **eq)}
    one_wg = dict(PRODUCT, B=1024)
    # ld = 448: 64 * 448 + 192 * 64 = 40960, ahead 4 at equality; one feature more: ahead 2
    assert ld_of(122) == 448 and 64 * 448 + 192 * 64 == AHEAD_LDS_MAX
    assert forms("build", max_features=122, n_select=64, **one_wg) == {AHEAD4}
    assert forms("build_lds_bytes", max_features=122, n_select=64, **one_wg) == {AHEAD_LDS_MAX}
    assert forms("build", max_features=122, n_select=65, **one_wg) == {AHEAD2}
    # ld = 1024: ahead 2 up to 42 measured features, plain from 43; ld = 1088: <2,2>
    assert (ld_of(334), ld_of(335)) == (1024, 1088)
    assert forms("build", max_features=334, n_select=42, **one_wg) == {AHEAD2}
    assert forms("build", max_features=334, n_select=43, **one_wg) == {AS14}
    assert forms("build", max_features=335, n_select=43, **one_wg) == {AS22}
    assert forms("build_threads", max_features=335, n_select=43, **one_wg) == {1024}
    # batch 1023 | 1024: 4 workgroups per sequence | one, and with it the ahead form
    assert forms("build_nsplit", max_features=100, n_select=64, **dict(PRODUCT, B=1023)) == {4}
    assert forms("build", max_features=100, n_select=64, **dict(PRODUCT, B=1023)) == {AS14}
    assert forms("build_nsplit", max_features=100, n_select=64, **one_wg) == {1}
    assert forms("build", max_features=100, n_select=64, **one_wg) == {AHEAD4}
    # 160 | more strips; 8 | 9, 13 | 14, 16 | 20 blocks
    b0 = KS_MAX_STRIPS // (ld_of(64) // 16)
    assert b0 * (ld_of(64) // 16) == KS_MAX_STRIPS and {b0, b0 + 1} <= set(batches_of(64))
    assert forms("fwd", max_features=64, n_select=64, **dict(PRODUCT, B=b0)) == {KSPLIT}
    assert forms("fwd", max_features=64, n_select=64, **dict(PRODUCT, B=b0 + 1)) == {LDS}
    one = dict(PRODUCT, B=1, max_features=334)
    assert [(p["nblk_max"], p["fwd"], p["fwd_nb"], p["chol"]) for ns in (128, 129, 208, 209, 256, 257) for _, p in rows(grid, n_select=ns, **one)] == [
        (8, KSPLIT, 0, LEFT), (9, LDS, 9, LEFT), (13, LDS, 13, LEFT), (14, GROUPED, 0, LEFT), (16, GROUPED, 0, LEFT), (20, GROUPED, 0, PANELS)]
    # the capacity edges: 676 | 677 slots, 512 | 513 measured features
    assert [(p["ld"], p["mld"], p["admitted"]) for mf, ns in ((676, 512), (677, 512), (676, 513)) for _, p in rows(grid, max_features=mf, n_select=ns, **dict(PRODUCT, B=1))] == [
        (2048, 1024, 1), (2112, 1024, 0), (2048, 1152, 0)]


def test_the_former_fall_through_launches_or_refuses(grid):
    """SL2_PANEL_FROM = 14 (TEST build) and 14 blocks: the one-launch form has no k_fwdsub_lds<14>.  The old code launched
    nothing and returned SL2_OK; the plan says grouped (mld = 448 is a multiple of 64)."""
    c = grid.compared()
    inp, got = c["changed_in"], c["changed_out"]
    assert len(inp) > 0
    assert (inp[:, IN.index("group_from")] == 14).all() and (got[:, OUT.index("nblk_max")] == 14).all()
    assert (got[:, OUT.index("mld")] == 448).all() and (got[:, OUT.index("fwd")] == GROUPED).all()
    assert (got[:, OUT.index("fwd_group_rows")] == np.where(inp[:, IN.index("fwd_group")] == 4, 4, 8)).all()
    assert set(inp[:, IN.index("superseded")].tolist()) == {0, 1}              # TEST build and product shape alike
    hit = [p for _, p in rows(grid, max_features=334, n_select=209, group_from=14, panel_from=14, fwd_variant=1, no_ksplit=1)]
    assert hit and all(p["nblk_max"] == 14 and p["fwd"] == GROUPED for p in hit)


def test_the_product_refuses_where_it_did(grid):
    """Without the superseded kernels: sl2_create refuses beyond 2048 state columns or 1024 rows and nowhere else; launch_update
    refuses - the factorisation first - exactly where neither product form applies, which no engine sl2_create admits with the
    product's knobs reaches."""
    seen = set()
    for inp, got in grid.chunks():
        o = {k: got[:, j] for j, k in enumerate(OUT)}
        prod = inp[:, IN.index("superseded")] == 0
        assert ((o["admitted"] == 1) == ((o["ld"] <= LD_MAX) & (o["mld"] <= MLD_MAX))).all()
        assert (o["error"][~prod] == 0).all()                                     # the TEST build has a kernel for everything
        assert ((o["error"] == 1) == (o["chol"] == CHOL_NONE)).all()
        assert ((o["error"] == 2) == ((o["chol"] != CHOL_NONE) & (o["fwd"] == FWD_NONE))).all()
        assert not np.isin(o["build"][prod], [TWO_PASS]).any() and not np.isin(o["chol"][prod], [PER_BLOCK]).any()
        assert not np.isin(o["fwd"][prod], [REREAD]).any()
        real = prod.copy()
        for k, v in PRODUCT.items():
            if k in ("build_variant", "chol_variant", "fwd_variant", "group_from", "panel_from"):   # what the product cannot set otherwise
                real &= inp[:, IN.index(k)] == v
        assert (o["error"][real] == 0).all()
        seen |= set(o["error"][prod].tolist())
    assert seen == {0, 1, 2}                                                      # both texts are reached by the grid


def test_equal_plans_are_equal_members_and_nothing_else():
    """operator== on the plans of a slice of the grid that holds every form: equal exactly where all nine members are."""
    P0 = OUT.index("build")
    inp = np.ascontiguousarray(np.concatenate([inputs_of(mf, ns) for mf, ns in ((5, 1), (100, 64), (122, 65), (334, 209), (335, 257), (677, 513))]))
    plans = [tuple(r) for r in uh.plans_of(inp)[:, P0:P0 + 9]]
    assert {p[0] for p in plans} == set(range(5)) and {p[4] for p in plans} == set(range(4)) and {p[6] for p in plans} == set(range(5))
    first = {}
    ref = [first.setdefault(p, k) for k, p in enumerate(plans)]
    assert uh.plans_equal(inp, ref).all()
    reps = sorted(first.values())
    print("update-plan equality: %d inputs, %d distinct plans" % (len(plans), len(reps)))
    assert len(reps) > 100
    reps = reps[::max(1, len(reps) // 300)]                 # every pair of some three hundred of them
    a = np.repeat(reps, len(reps))
    b = np.tile(reps, len(reps))
    keep = a != b
    both = np.ascontiguousarray(np.concatenate([inp[a[keep]], inp[b[keep]]]))
    k = int(keep.sum())
    assert not uh.plans_equal(both, list(range(k, 2 * k)))[:k].any()
