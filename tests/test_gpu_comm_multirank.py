"""The multi-rank branches of scenelib2_amd/csrc/sl2_comm.hip, on ONE device.

RCCL refuses two ranks of a clique on the same GPU, so over RCCL a one-GPU box only ever runs the "root copies its own block"
branch of sl2_scatter_frames and an identity all-gather.  scenelib2_amd/libscenelib2_amd_comm_test.so is the product's own
sl2_comm.o linked over tests/rccl_standin.cpp in place of librccl (the stand-in's semantics are described at its top): with it
2 .. 4 ranks live on device 0 and the project's own code runs - the per-destination offsets, which ranks skip an empty block,
a root other than rank 0, the grouped form one host thread needs and the thread-per-rank form, the ordering behind the streams,
and the claim that row r * batch + b of the gather is global sequence r * batch + b on every rank.

References: NumPy slicing with scenelib2_amd.sharding.shard_range (scatter, exactly), rows built from each engine's accessors
(gather, exactly), the CPU oracle and a single engine of batch 6 (end to end, TOL_X / TOL_P of tests/test_gpu_slam.py).
NOT covered here or anywhere: RCCL itself with more than one rank (xGMI), and any scaling figure.

The only waits are the stand-in's rendezvous bound (20 s) and the joins of the rank threads; both fail the test."""
import ctypes as C
import os
import threading
import time
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import rel_fro
from slam_helpers import Pair, compare_state
from scenelib2_amd import Engine, _lib, sharding, synth
from test_gpu_slam import TOL_P, TOL_X
from test_gpu_slot_squeeze import _gather_expected, _retire

pytestmark = pytest.mark.gpu

CANARY = 0xC5
TAIL = 64
JOIN_SECONDS = 60.0          # well above TWO rendezvous bounds of the stand-in (ncclCommInitRank, then the collective): a peer
                             # that never calls shows as the stand-in's error, not as a thread that did not finish
D2D = 3                      # hipMemcpyDeviceToDevice
NON_BLOCKING = 1             # hipStreamNonBlocking: no implicit ordering with the NULL stream to hide a wrong stream behind
N_SLOTS = 12
RETIRED = [3, 7]             # slots retired in sequence 0 of rank 1: zeros in the middle of a map row


@pytest.fixture(scope="module")
def env():
    """The test build of the communication library, the HIP runtime and four streams of device 0."""
    _lib.load()                 # the engine library first: the communication library links it
    L = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libscenelib2_amd_comm_test.so"))
    vp = C.c_void_p
    L.sl2_comm_last_error.restype = C.c_char_p
    L.sl2_comm_unique_id.argtypes = [vp]
    L.sl2_comm_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.sl2_comm_create_all.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]
    L.sl2_comm_destroy.argtypes = [vp]
    L.sl2_comm_destroy.restype = None
    L.sl2_scatter_frames.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, vp, vp]
    L.sl2_gather_states.argtypes = [vp, vp, C.c_int, vp, vp]
    L.sl2_gather_row_doubles.argtypes = [C.c_int, C.c_int]
    hip = C.CDLL("libamdhip64.so")                                    # the runtime the libraries are linked against
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
    hip.hipStreamDestroy.argtypes = [vp]
    hip.hipStreamSynchronize.argtypes = [vp]
    hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    streams = []
    for _ in range(4):
        st = vp()
        assert hip.hipStreamCreateWithFlags(C.byref(st), NON_BLOCKING) == 0
        streams.append(st.value)
    yield SimpleNamespace(L=L, hip=hip, streams=streams)
    for st in streams:
        hip.hipStreamDestroy(st)


@pytest.fixture(autouse=True)
def no_communicator_outlives_its_test(env):
    assert env.L.sl2_standin_live_comms() == 0
    yield
    assert env.L.sl2_standin_live_comms() == 0


def _err(L):
    return (L.sl2_comm_last_error() or b"").decode("utf-8", "replace")


def _create_all(L, n):
    comms = (C.c_void_p * n)()
    assert L.sl2_comm_create_all(n, (C.c_int * n)(*([0] * n)), comms) == 0, _err(L)
    assert L.sl2_standin_live_comms() == n              # the stand-in's communicators, not RCCL's
    return list(comms)


def _destroy(L, comms):
    for c in comms:
        if c:
            L.sl2_comm_destroy(c)


def _sync(env, streams):
    for st in streams:
        assert env.hip.hipStreamSynchronize(st) == 0


def _run_ranks(n, body):
    """body(rank) on n host threads; a thread that has not finished in JOIN_SECONDS fails the test."""
    results = [None] * n

    def run(r):
        try:
            results[r] = body(r)
        except BaseException as e:       # handed to the test's own thread
            results[r] = e
    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(n)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_SECONDS
    for r, t in enumerate(threads):
        t.join(max(0.0, deadline - time.monotonic()))
        assert not t.is_alive(), "the thread of rank %d did not finish in %g s" % (r, JOIN_SECONDS)
    for res in results:
        if isinstance(res, BaseException):
            raise res
    return results


# ------------------------------------------------------------------------------------------------ a. scatter

class _ScatterBuffers:
    """`total` random frames on the root, and per rank count * frame_bytes bytes + TAIL, all bytes CANARY."""

    def __init__(self, nranks, total, frame_bytes, seed, sources=1):
        rng = np.random.RandomState(seed)
        self.ranges = [sharding.shard_range(total, nranks, r) for r in range(nranks)]
        self.fb = frame_bytes
        self.src = [rng.randint(0, 256, (total, frame_bytes)).astype(np.uint8) for _ in range(sources)]
        self.src_dev = [_lib.DeviceBuffer(max(s.nbytes, 1)) for s in self.src]
        for s, d in zip(self.src, self.src_dev):
            if s.nbytes:
                d.upload(s)
        self.recv = [_lib.DeviceBuffer(n * frame_bytes + TAIL) for _, n in self.ranges]
        for d in self.recv:
            d.upload(np.full(d.nbytes, CANARY, dtype=np.uint8))

    def check(self, bufs, src):
        for r, (first, count) in enumerate(self.ranges):
            got = bufs[r].download((count * self.fb + TAIL,), np.uint8)
            assert np.array_equal(got[:count * self.fb].reshape(count, self.fb), src[first:first + count]), "block of rank %d" % r
            assert (got[count * self.fb:] == CANARY).all(), "canary of rank %d" % r

    def free(self):
        for d in self.src_dev + self.recv:
            d.free()


def _scatter(env, comm, rank, root, bufs, src_dev, total, stream):
    src = C.c_void_p(src_dev.ptr) if rank == root else None      # frames_all exists on the root only
    return env.L.sl2_scatter_frames(comm, root, src, bufs.fb, total, C.c_void_p(bufs.recv[rank].ptr), stream)


@pytest.mark.parametrize("total", [0, 1, 2, 3, 5, 7])
@pytest.mark.parametrize("frame_bytes", [77, 320 * 240])
@pytest.mark.parametrize("root_is_last", [False, True], ids=["root0", "rootlast"])
@pytest.mark.parametrize("nranks", [2, 3, 4])
@pytest.mark.parametrize("form", ["grouped", "threads"])
def test_scatter_equals_numpy_slicing(env, form, nranks, root_is_last, frame_bytes, total):
    """Rank r's buffer is src[first_r : first_r + count_r] of the root's frames, exactly, and nothing behind it is written:
    (first_r, count_r) from the Python launcher's shard_range, not from the library.  total < nranks leaves empty ranks on
    both sides of the root and a root with an empty block; 5 and 7 give sizes that differ by one.  grouped: ncclCommInitAll,
    one host thread, all ranks' calls inside sl2_comm_group_begin / _end.  threads: sl2_comm_unique_id, sl2_comm_create and
    the scatter from one host thread per rank, no outer group (examples/sharded_monoslam.cpp)."""
    L = env.L
    root = nranks - 1 if root_is_last else 0
    bufs = _ScatterBuffers(nranks, total, frame_bytes, seed=1000 * nranks + 10 * total + root)
    comms = [None] * nranks
    try:
        if form == "grouped":
            comms = _create_all(L, nranks)
            assert L.sl2_comm_group_begin() == 0
            for r in range(nranks):
                assert _scatter(env, comms[r], r, root, bufs, bufs.src_dev[0], total, env.streams[r]) == 0, _err(L)
            assert L.sl2_comm_group_end() == 0, _err(L)
            _sync(env, env.streams[:nranks])
        else:
            ident = (C.c_ubyte * 128)()
            assert L.sl2_comm_unique_id(ident) == 0, _err(L)

            def body(r):
                c = C.c_void_p()
                assert L.sl2_comm_create(ident, nranks, r, 0, C.byref(c)) == 0, _err(L)
                comms[r] = c
                assert L.sl2_comm_rank(c) == r and L.sl2_comm_nranks(c) == nranks
                assert _scatter(env, c, r, root, bufs, bufs.src_dev[0], total, env.streams[r]) == 0, _err(L)
                _sync(env, [env.streams[r]])
            _run_ranks(nranks, body)
            assert L.sl2_standin_live_comms() == nranks
        bufs.check(bufs.recv, bufs.src[0])
    finally:
        _destroy(L, comms)
        bufs.free()


@pytest.mark.parametrize("streams", ["null", "shared"])
def test_scatter_on_the_null_stream_and_on_one_stream_for_all_ranks(env, streams):
    """Three ranks, root 1, five frames, grouped: every rank on the NULL stream, and every rank on the same stream."""
    L = env.L
    bufs = _ScatterBuffers(3, 5, 77, seed=31)
    comms = _create_all(L, 3)
    st = None if streams == "null" else env.streams[0]
    try:
        assert L.sl2_comm_group_begin() == 0
        for r in range(3):
            assert _scatter(env, comms[r], r, 1, bufs, bufs.src_dev[0], 5, st) == 0, _err(L)
        assert L.sl2_comm_group_end() == 0, _err(L)
        _sync(env, [st])
        bufs.check(bufs.recv, bufs.src[0])
    finally:
        _destroy(L, comms)
        bufs.free()


# ------------------------------------------------------------------------------------------------ b. stream order

def test_scatter_is_ordered_on_the_stream_it_was_given(env):
    """Two scatters of different sources back to back on the same (non-blocking) streams, a device copy of recv to a side
    buffer queued between them, one synchronisation at the end: the side buffers hold the first source's blocks, recv the
    second's.  Three ranks, root 1, five frames of 320 x 240."""
    L, fb, total = env.L, 320 * 240, 5
    bufs = _ScatterBuffers(3, total, fb, seed=47, sources=2)
    assert not np.array_equal(bufs.src[0], bufs.src[1])
    side = [_lib.DeviceBuffer(d.nbytes) for d in bufs.recv]
    for d in side:
        d.upload(np.zeros(d.nbytes, dtype=np.uint8))
    comms = _create_all(L, 3)
    try:
        for k in range(2):
            assert L.sl2_comm_group_begin() == 0
            for r in range(3):
                assert _scatter(env, comms[r], r, 1, bufs, bufs.src_dev[k], total, env.streams[r]) == 0, _err(L)
            assert L.sl2_comm_group_end() == 0, _err(L)
            if k == 0:
                for r in range(3):
                    assert env.hip.hipMemcpyAsync(side[r].ptr, bufs.recv[r].ptr, side[r].nbytes, D2D, env.streams[r]) == 0
        _sync(env, env.streams[:3])
        bufs.check(side, bufs.src[0])
        bufs.check(bufs.recv, bufs.src[1])
    finally:
        _destroy(L, comms)
        for d in side:
            d.free()
        bufs.free()


# ------------------------------------------------------------------------------------------------ c, d. gather

class _ThreeRanks:
    """Six different sequences (one Pair without an engine: frames and six oracles) on three engines of batch 2, all on
    device 0, and a three-rank communicator."""

    def __init__(self, env, n_frames):
        self.env = env
        self.big = Pair(N_SLOTS, n_frames, batch=6, make_engine=False)
        self.engines = [self.big.make_engine_for(2 * r, 2, N_SLOTS) for r in range(3)]
        self.comms = _create_all(env.L, 3)
        self.out = {}

    def frames(self, r, k):
        return np.stack([self.big.frames[2 * r + b][k] for b in range(2)])

    def step_host(self, k):
        for r, eng in enumerate(self.engines):
            eng.go_one_step(self.frames(r, k))

    def prepare(self, what):
        """Every rank's out allocated and filled with NaN (host-synchronous copies: NOT to be called between a queued step
        and its gather)."""
        row = self.env.L.sl2_gather_row_doubles(what, N_SLOTS)
        if what not in self.out:
            self.out[what] = [_lib.DeviceBuffer(8 * row * 6) for _ in range(3)]
        for d in self.out[what]:
            d.upload(np.full(6 * row, np.nan))

    def gather(self, what, streams, prepared=False, first=None):
        """sl2_gather_states of every rank, grouped, rank r on streams[r] into its own out: [rank][6][row] after one sync.
        first(r), if given, is called inside the group right before rank r's gather (work to queue on its engine).  With
        prepared=True nothing but `first` and the gather calls happens before the synchronisation at the end."""
        L = self.env.L
        if not prepared:
            self.prepare(what)
        out = self.out[what]
        assert L.sl2_comm_group_begin() == 0
        for r in range(3):
            if first is not None:
                first(r)
            assert L.sl2_gather_states(self.comms[r], self.engines[r].h, what, C.c_void_p(out[r].ptr), streams[r]) == 0, _err(L)
        assert L.sl2_comm_group_end() == 0, _err(L)
        _sync(self.env, streams)
        row = L.sl2_gather_row_doubles(what, N_SLOTS)
        return [d.download((6, row), np.float64) for d in out]

    def expected(self, what):
        return np.concatenate([_gather_expected(eng, what, N_SLOTS, 2) for eng in self.engines], axis=0)

    def close(self):
        _destroy(self.env.L, self.comms)
        for bufs in self.out.values():
            for d in bufs:
                d.free()
        for eng in self.engines:
            eng.close()


def test_gather_is_in_rank_order_and_identical_on_every_rank(env):
    """Three ranks x batch 2 x 12 slots, two slots retired in sequence 0 of rank 1, two steps; then every kind, grouped, each
    rank on its own stream with its own out.  Every rank's out equals the rows built in NumPy from each engine's accessors,
    concatenated in rank order - row r * 2 + b is sequence b of rank r - and so every rank's out equals the others'."""
    w = _ThreeRanks(env, n_frames=2)
    try:
        _retire(w.engines[1], [RETIRED, []])
        for k in range(2):
            w.step_host(k)
        for what in (0, 1, 2):
            want = w.expected(what)
            assert len({want[i, :13].tobytes() for i in range(6)}) == 6          # six different sequences: a wrong order shows
            got = w.gather(what, env.streams[:3])
            for r in range(3):
                assert np.array_equal(got[r], want), (what, r, np.argwhere((got[r] != want).any(axis=1)).ravel())
                assert np.array_equal(got[r], got[0]), (what, r)
            if what == 2:
                y = want[2, 13:].reshape(N_SLOTS, 3)
                assert [s for s in range(N_SLOTS) if not y[s].any()] == RETIRED          # zeros in the middle of the row
    finally:
        w.close()


def test_one_rank_gather_over_the_stand_in_equals_the_gather_over_rccl(env):
    """The anchor where RCCL can run: one rank, the same engine, every kind through the stand-in library and through the
    product library (real ncclCommInitAll / ncclAllGather on one device): equal, and equal to the accessors' rows."""
    L = env.L
    R = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libscenelib2_amd_comm.so"))
    R.sl2_comm_last_error.restype = C.c_char_p
    R.sl2_comm_create_all.argtypes = L.sl2_comm_create_all.argtypes
    R.sl2_gather_states.argtypes = L.sl2_gather_states.argtypes
    R.sl2_comm_destroy.argtypes = [C.c_void_p]
    R.sl2_comm_destroy.restype = None
    big = Pair(N_SLOTS, 2, batch=2, make_engine=False)
    eng = big.make_engine_for(0, 2, N_SLOTS)
    real = (C.c_void_p * 1)()
    assert R.sl2_comm_create_all(1, None, real) == 0, _err(R)
    assert L.sl2_standin_live_comms() == 0                           # (that one was RCCL's)
    mine = _create_all(L, 1)
    try:
        _retire(eng, [RETIRED, []])
        for k in range(2):
            eng.go_one_step(big.frame_batch(k))
        for what in (0, 1, 2):
            row = L.sl2_gather_row_doubles(what, N_SLOTS)
            got = []
            for lib, comm in ((L, mine[0]), (R, real[0])):
                out = _lib.DeviceBuffer(8 * row * 2)
                try:
                    out.upload(np.full(2 * row, np.nan))
                    assert lib.sl2_gather_states(comm, eng.h, what, C.c_void_p(out.ptr), env.streams[0]) == 0, _err(lib)
                    _sync(env, [env.streams[0]])
                    got.append(out.download((2, row), np.float64))
                finally:
                    out.free()
            assert np.array_equal(got[0], got[1]), what
            assert np.array_equal(got[0], _gather_expected(eng, what, N_SLOTS, 2)), what
    finally:
        _destroy(L, mine)
        R.sl2_comm_destroy(real[0])
        eng.close()


def test_gather_is_ordered_behind_the_engines_queued_step(env):
    """Three steps per engine on frames that are already on the device (queued, not waited for) and at once the gather, on
    ANOTHER, non-blocking stream: the rows are those of the state after the steps.  Between the first sl2_go_one_step and
    the last sl2_gather_states there is no copy, no accessor and no synchronisation (the outs are filled with NaN before);
    the one thing that orders the pack kernel behind the steps is the event sl2_gather_states records on the engine's
    stream and makes the given stream wait for."""
    n_queued, what = 3, 2
    w = _ThreeRanks(env, n_frames=1 + n_queued)
    dev = [[_lib.DeviceBuffer(2 * 320 * 240) for _ in range(n_queued)] for _ in range(3)]
    try:
        _retire(w.engines[1], [RETIRED, []])
        w.step_host(0)
        for r in range(3):
            for k in range(n_queued):
                dev[r][k].upload(w.frames(r, 1 + k))
        before = w.gather(what, env.streams[:3])[0]
        w.prepare(what)
        for eng in w.engines:
            eng.synchronize()

        def queue_steps(r):
            for k in range(n_queued):
                w.engines[r].go_one_step(dev[r][k].ptr, on_device=True)
        got = w.gather(what, env.streams[:3], prepared=True, first=queue_steps)
        want = w.expected(what)                                       # (the accessors synchronise the engines)
        assert all((before[i] != want[i]).any() for i in range(6)), "the steps must move every sequence"
        for r in range(3):
            assert np.array_equal(got[r], want), (r, np.argwhere((got[r] != want).any(axis=1)).ravel())
    finally:
        w.close()
        for d in sum(dev, []):
            d.free()


# ------------------------------------------------------------------------------------------------ e. end to end

def _same_measurements(e1, b1, e2, b2):
    """z, selection and counters of sequence b1 of engine e1 and sequence b2 of engine e2: equal."""
    s1, c1 = e1.selection(b1)
    s2, c2 = e2.selection(b2)
    assert list(s1) == list(s2) and c1 == c2
    f1, f2 = e1.features(b1), e2.features(b2)
    assert len(f1) == len(f2)
    for a, b in zip(f1, f2):
        assert (a["label"], a["attempted"], a["successful"], a["selected"], a["success"]) == \
               (b["label"], b["attempted"], b["successful"], b["selected"], b["success"])
        assert np.array_equal(a["z"], b["z"])


def test_scatter_step_gather_against_the_oracle_and_a_single_engine(env):
    """Three ranks x batch 2, four frames.  Each step's six frames are on rank 1 only; they are scattered (grouped, every rank
    on its engine's stream), each engine steps its block from device memory, and at the end xv and Pxx are gathered.  Against
    six oracles fed the same frames (TOL_X / TOL_P), and against ONE engine of batch 6 stepping the same frames: z, selection
    and counters equal, state to the same tolerances (kernel dispatch depends on the batch: no bit-equality promised)."""
    L, fb, n_frames, root = env.L, 320 * 240, 4, 1
    w = _ThreeRanks(env, n_frames)
    single = w.big.make_engine_for(0, 6, N_SLOTS)
    staged = [_lib.DeviceBuffer(6 * fb) for _ in range(n_frames)]      # on the root: one buffer per step, none reused
    mine = [_lib.DeviceBuffer(2 * fb) for _ in range(3)]
    try:
        for k in range(n_frames):
            staged[k].upload(w.big.frame_batch(k))
        streams = [eng.stream for eng in w.engines]
        for k in range(n_frames):
            assert L.sl2_comm_group_begin() == 0
            for r in range(3):
                src = C.c_void_p(staged[k].ptr) if r == root else None
                assert L.sl2_scatter_frames(w.comms[r], root, src, fb, 6, C.c_void_p(mine[r].ptr), streams[r]) == 0, _err(L)
            assert L.sl2_comm_group_end() == 0, _err(L)
            for r, eng in enumerate(w.engines):
                eng.go_one_step(mine[r].ptr, on_device=True)
        rows = w.gather(1, streams)
        for k in range(n_frames):
            for b, s in enumerate(w.big.oracles):
                s.go_one_step(w.big.frames[b][k], False)
            single.go_one_step(w.big.frame_batch(k))
        for r in range(1, 3):
            assert np.array_equal(rows[r], rows[0])
        assert np.array_equal(rows[0], w.expected(1))
        worst = dict(x=0.0, P=0.0)
        for g, s in enumerate(w.big.oracles):
            xv, Pxx = s.get_state()
            dx, dP = np.abs(rows[0][g, :13] - xv).max(), rel_fro(rows[0][g, 13:].reshape(13, 13), Pxx)
            worst = dict(x=max(worst["x"], dx), P=max(worst["P"], dP))
            assert dx <= TOL_X and dP <= TOL_P, (g, dx, dP)
        # the whole state, z, selection and counters of every engine against its oracles (compare_state's assertions)
        for r, eng in enumerate(w.engines):
            compare_state(w.big.oracles[2 * r:2 * r + 2], eng, TOL_X, TOL_P)
        compare_state(w.big.oracles, single, TOL_X, TOL_P)
        for g in range(6):
            eng, b = w.engines[g // 2], g % 2
            _same_measurements(eng, b, single, g)
            dx = np.abs(eng.total_state(b) - single.total_state(g)).max()
            dP = rel_fro(eng.total_covariance(b), single.total_covariance(g))
            assert dx <= TOL_X and dP <= TOL_P, (g, dx, dP)
        print("sharded 3 x 2 against the oracles: worst |dxv| = %.3e, worst rel |dPxx| = %.3e" % (worst["x"], worst["P"]))
    finally:
        w.close()
        single.close()
        for d in staged + mine:
            d.free()


# ------------------------------------------------------------------------------------------------ f. misuse

def _bare_engine(batch):
    return Engine(synth.default_camera(), synth.default_params(N_SLOTS), batch, N_SLOTS)


@pytest.mark.parametrize("form", ["grouped", "threads"])
def test_gather_of_engines_with_different_batches_is_refused(env, form):
    """Two ranks whose engines hold 2 and 3 sequences: RCCL would hang or write past `out`; the stand-in compares the counts,
    and the library hands that on - a non-zero status whose text names ncclAllGather.  grouped: the status of
    sl2_comm_group_end (the calls inside a group only queue).  threads: the status of sl2_gather_states itself."""
    L = env.L
    engines = [_bare_engine(2), _bare_engine(3)]
    out = [_lib.DeviceBuffer(8 * 13 * 6) for _ in range(2)]
    comms = _create_all(L, 2)
    try:
        if form == "grouped":
            assert L.sl2_comm_group_begin() == 0
            for r in range(2):
                assert L.sl2_gather_states(comms[r], engines[r].h, 0, C.c_void_p(out[r].ptr), env.streams[r]) == 0, _err(L)
            assert L.sl2_comm_group_end() != 0
            assert "ncclAllGather" in _err(L), _err(L)
        else:
            def body(r):
                rc = L.sl2_gather_states(comms[r], engines[r].h, 0, C.c_void_p(out[r].ptr), env.streams[r])
                return rc, _err(L)
            for rc, text in _run_ranks(2, body):
                assert rc != 0 and "ncclAllGather" in text, (rc, text)
        _sync(env, env.streams[:2])
    finally:
        _destroy(L, comms)
        for d in out:
            d.free()
        for e in engines:
            e.close()


def test_a_rank_that_joins_its_clique_twice_is_refused(env):
    """sl2_comm_create for rank 0 of 2 waits on a thread; a second rank 0 under the same id is refused at once (RCCL would
    hang), names the cause, and leaves the clique whole: rank 1 then joins and both calls succeed."""
    L = env.L
    ident = (C.c_ubyte * 128)()
    assert L.sl2_comm_unique_id(ident) == 0, _err(L)
    comms = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    rc0 = []
    t = threading.Thread(target=lambda: rc0.append(L.sl2_comm_create(ident, 2, 0, 0, C.byref(comms[0]))), daemon=True)
    t.start()
    try:
        deadline = time.monotonic() + JOIN_SECONDS
        while L.sl2_standin_live_comms() < 1 and time.monotonic() < deadline:       # until rank 0 has arrived
            time.sleep(0)
        assert L.sl2_standin_live_comms() == 1
        assert L.sl2_comm_create(ident, 2, 0, 0, C.byref(comms[2])) != 0 and "already joined" in _err(L), _err(L)
        assert not comms[2] and L.sl2_standin_live_comms() == 1
        assert L.sl2_comm_create(ident, 2, 1, 0, C.byref(comms[1])) == 0, _err(L)
        t.join(JOIN_SECONDS)
        assert not t.is_alive() and rc0 == [0]
    finally:
        _destroy(L, comms)


def test_scatter_whose_ranks_disagree_on_the_total_is_refused(env):
    """Root 0 scatters five sequences over two ranks (3 + 2), rank 1 believes in three (2 + 1): the send and the receive differ
    in their byte counts.  Refused at sl2_comm_group_end, nothing copied."""
    L = env.L
    bufs = _ScatterBuffers(2, 5, 77, seed=5)
    comms = _create_all(L, 2)
    try:
        assert L.sl2_comm_group_begin() == 0
        assert _scatter(env, comms[0], 0, 0, bufs, bufs.src_dev[0], 5, env.streams[0]) == 0, _err(L)
        assert _scatter(env, comms[1], 1, 0, bufs, bufs.src_dev[0], 3, env.streams[1]) == 0, _err(L)
        assert L.sl2_comm_group_end() != 0
        assert "byte counts" in _err(L), _err(L)
        _sync(env, env.streams[:2])
        got = bufs.recv[1].download((bufs.recv[1].nbytes,), np.uint8)
        assert (got == CANARY).all()
        assert L.sl2_comm_group_end() != 0                            # and an end without a begin
    finally:
        _destroy(L, comms)
        bufs.free()


def test_gather_refuses_an_unknown_kind_and_with_two_devices_an_engine_of_another_device(env):
    """An unknown kind and a NULL out are refused, and the communicator stays usable.  The refusal of an engine that lives on
    another device than the communicator RUNS ONLY WHERE THERE ARE TWO DEVICES: with one, neither a communicator nor an engine
    of device 1 can exist, so no mismatched pair can be put together (what is asserted then is only that
    sl2_comm_create_all refuses device 1) and that line of sl2_gather_states stays unexecuted by the suite."""
    L = env.L
    eng = _bare_engine(2)
    out = _lib.DeviceBuffer(8 * 182 * 2)
    comms = _create_all(L, 1)
    other = None
    try:
        assert L.sl2_gather_states(comms[0], eng.h, 3, C.c_void_p(out.ptr), None) == 1 and "unknown kind" in _err(L)
        assert L.sl2_gather_states(comms[0], eng.h, -1, C.c_void_p(out.ptr), None) == 1
        assert L.sl2_gather_states(comms[0], eng.h, 0, None, None) == 1
        if _lib.device_count() >= 2:
            other = Engine(eng.cam, eng.params, 2, N_SLOTS, device=1)
            assert L.sl2_gather_states(comms[0], other.h, 0, C.c_void_p(out.ptr), None) == 1 and "another device" in _err(L)
        else:
            # one device: a communicator of device 1 cannot exist (and neither can an engine), so no mismatched pair can be
            # put together; the refusal itself runs where there are two devices
            c = (C.c_void_p * 1)()
            assert L.sl2_comm_create_all(1, (C.c_int * 1)(1), c) == 1 and not c[0]
        assert L.sl2_gather_states(comms[0], eng.h, 0, C.c_void_p(out.ptr), None) == 0, _err(L)       # still usable
        eng.synchronize()
        _sync(env, [None])
    finally:
        _destroy(L, comms)
        out.free()
        eng.close()
        if other is not None:
            other.close()
