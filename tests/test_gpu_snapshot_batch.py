"""sl2_snapshot_batch (include/scenelib2_amd.h): the public state of a RANGE of sequences in one call.

The reference is sl2_snapshot itself (tests/test_gpu_snapshot.py holds it to the accessors): with SL2_SNAP_ALL blob i of a batch
call must be BYTE FOR BYTE what sl2_snapshot returns for sequence seq0 + i under the same cursors; with fewer sections every
section present must be the same section of that blob.  Everything here is exact equality - the call computes nothing.
Offsets: offsets[0] = 0, each step is header.bytes rounded up to 16, the padding is zero, nothing at or behind offsets[nseq] is
written (a 0xA5 pattern behind it survives)."""
import ctypes as C

import numpy as np
import pytest

from mapping_helpers import make_mapping_sequence
from scenelib2_amd import Engine, _lib, decode_snapshot
from slam_helpers import Pair

pytestmark = pytest.mark.gpu

ALL = _lib.SL2_SNAP_ALL
FEATURES, COV, SELECTION, TRAJ, PARTIAL, PATCHES = 1, 2, 4, 8, 16, 32
INT32_MAX = 2 ** 31 - 1
SENTINEL = 0xA5
SCAN_CHUNK = 256                                  # kScanChunk of sl2_snapshot.hip
SECTION_ORDER = ("features", "cov", "selection", "traj", "partial", "patches")
SECTION_BIT = dict(features=FEATURES, cov=COV, selection=SELECTION, traj=TRAJ, partial=PARTIAL, patches=PATCHES)


def header(blob):
    return _lib.sl2_snapshot_header.from_buffer_copy(blob[:256])


def single_raw(e, seq, traj_cursor=0, patch_from_label=0):
    """The bytes of sl2_snapshot for one sequence."""
    blob, n = _lib.vp(), C.c_size_t(0)
    _lib.check(e.L.sl2_snapshot(e.h, int(seq), int(traj_cursor), int(patch_from_label), C.byref(blob), C.byref(n)), e.L)
    return C.string_at(blob.value, n.value)


def batch_call(e, seq0, nseq, sections=ALL, cursors=None, out_bytes=None, slack=256):
    """sl2_snapshot_batch, host form, into a buffer filled with the sentinel: (rc, buffer, offsets).  out_bytes = what the
    call is TOLD the buffer holds (default: nseq bounds); the buffer itself is `slack` bytes longer."""
    told = e.snapshot_bound(sections) * nseq if out_bytes is None else int(out_bytes)
    buf = np.full(max(told, e.snapshot_bound(sections) * nseq) + slack, SENTINEL, dtype=np.uint8)
    offs = np.full(nseq + 1, 2 ** 64 - 1, dtype=np.uint64)
    cur = None if cursors is None else np.ascontiguousarray(cursors, dtype=np.int32).reshape(nseq, 2)
    rc = e.L.sl2_snapshot_batch(e.h, seq0, nseq, sections, None if cur is None else cur.ctypes.data_as(_lib.vp),
                                buf.ctypes.data_as(_lib.vp), told, offs.ctypes.data_as(_lib.vp), 0)
    return rc, buf, offs


def check_packing(buf, offs, nseq):
    """The offset rules; returns the blobs (header.bytes long each)."""
    assert int(offs[0]) == 0
    blobs = []
    for i in range(nseq):
        at, nxt = int(offs[i]), int(offs[i + 1])
        h = header(buf[at:at + 256].tobytes())
        assert h.magic == 0x53324C53 and nxt - at == (h.bytes + 15) & ~15 and nxt > at, i
        assert not buf[at + h.bytes:nxt].any(), "padding of blob %d" % i
        blobs.append(buf[at:at + h.bytes].tobytes())
    assert (buf[int(offs[nseq]):] == SENTINEL).all(), "bytes at or behind offsets[nseq] were written"
    return blobs


def assert_identity(e, seq0, nseq, cursors=None):
    """SL2_SNAP_ALL over [seq0, seq0 + nseq): packing rules, and every blob the bytes of sl2_snapshot."""
    rc, buf, offs = batch_call(e, seq0, nseq, ALL, cursors)
    assert rc == _lib.SL2_OK, e.L.sl2_last_error()
    blobs = check_packing(buf, offs, nseq)
    for i, blob in enumerate(blobs):
        tc, pl = (0, 0) if cursors is None else cursors[i]
        assert blob == single_raw(e, seq0 + i, tc, pl), "blob %d (sequence %d)" % (i, seq0 + i)
        assert header(blob).seq == seq0 + i and header(blob).omitted_sections == 0
    return blobs, offs


# ------------------------------------------------------------------------------------------------- the unequal five
CURSORS5 = [(0, 0), (3, 2), (10 ** 6, 0), (0, INT32_MAX), (5, 7)]      # (traj_cursor, patch_from_label); 10^6 is beyond traj_total


@pytest.fixture(scope="module")
def five():
    """Batch 5, 16 feature slots, mapping on, a dozen steps: partial features, particles and fresh templates exist.  The
    sequences are made unequal: 1 loses two features, 2 sits out the second half of the steps, 3 is reset (an empty map)."""
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=40)
    B = 5
    e = Engine(cam, params, B, 16)
    e.set_vehicle_state(np.tile(spec.xv0, (B, 1)), np.tile(spec.Pxx0, (B, 1, 1)))
    e.add_known_features(np.tile(spec.feat_y, (B, 1, 1)), np.tile(spec.xp_org(), (B, 1, 1)), np.tile(templates, (B, 1, 1, 1)))
    steps = 0
    for k in range(1, 41):      # a dozen steps, then on until a partially initialised feature with its particles is in flight
        if k == 7:
            e.set_active([1, 1, 0, 1, 1])
        e.go_one_step(np.tile(frames[k], (B, 1, 1)), save_trajectory=True, enable_mapping=True)
        steps = k
        if k >= 12 and e.partial_feature(0)["pf"] is not None:
            break
    labels = [f["label"] for f in e.features(1) if f["fully_initialised"]]
    assert e.delete_features([-1, labels[1], -1, -1, -1])[1] and e.delete_features([-1, labels[3], -1, -1, -1])[1]
    e.reset_sequences(3, 1)
    heads = [header(single_raw(e, b)) for b in range(B)]
    assert heads[3].n_features == 0 and heads[1].n_features == heads[0].n_features - 2
    assert heads[2].traj_total == 6 and heads[0].traj_total == steps >= 12
    assert heads[0].n_partial > 0 and len({h.bytes for h in heads}) >= 4      # the sizes differ: the offsets matter
    yield e
    e.close()


@pytest.mark.parametrize("seq0,nseq", [(0, 5), (1, 3), (4, 1)])
def test_blobs_are_the_single_calls_bytes(five, seq0, nseq):
    blobs, _ = assert_identity(five, seq0, nseq, CURSORS5[seq0:seq0 + nseq])
    if seq0 == 0:
        heads = [header(b) for b in blobs]
        assert heads[2].traj_count == 0 and heads[2].traj_first == heads[2].traj_total      # the cursor beyond traj_total
        assert heads[3].n_patches == 0 and heads[0].n_patches == heads[0].n_features > 0
        assert heads[1].traj_first == 3 and heads[4].traj_first == 5
    assert_identity(five, seq0, nseq, None)      # NULL cursors = (0, 0) for all


def section_bytes(blob):
    """Name -> the bytes of each section of a blob, walked by the header's offsets."""
    h = header(blob)
    offs = [h.off_features, h.off_cov, h.off_selection, h.off_traj, h.off_partial, h.off_patches, h.bytes]
    assert h.off_xv == 256 and h.off_Pxx == 256 + 104 and h.off_features == 256 + 104 + 1352 and offs == sorted(offs)
    out = dict(pose=blob[256:h.off_features])
    for k, name in enumerate(SECTION_ORDER):
        out[name] = blob[offs[k]:offs[k + 1]]
    return out


SECTION_SETS = [0] + [b for b in (FEATURES, SELECTION, TRAJ, PARTIAL, PATCHES)] + \
               [ALL & ~b for b in (COV, SELECTION, TRAJ, PARTIAL, PATCHES)] + [ALL & ~(FEATURES | COV), FEATURES | SELECTION]


@pytest.mark.parametrize("sections", SECTION_SETS)
def test_sections(five, sections):
    """POSE only, each section alone, SL2_SNAP_ALL less each one section.  (COV alone and ALL less FEATURES are the refused
    combination - COV without FEATURES -, see the next test; ALL less FEATURES and COV stands in.)"""
    e = five
    full, _ = assert_identity(e, 0, 5, CURSORS5)
    rc, buf, offs = batch_call(e, 0, 5, sections, CURSORS5)
    assert rc == _lib.SL2_OK
    blobs = check_packing(buf, offs, 5)
    for i in range(5):
        hf, hp = header(full[i]), header(blobs[i])
        sf, sp = section_bytes(full[i]), section_bytes(blobs[i])
        assert hp.omitted_sections == ALL & ~sections and hp.bytes <= e.snapshot_bound(sections)
        assert sp["pose"] == sf["pose"] and len(sp["pose"]) == 8 * (13 + 169)
        for name in SECTION_ORDER:
            assert sp[name] == (sf[name] if sections & SECTION_BIT[name] else b""), (i, name)
        # what describes the sequence stays true, what describes the blob follows the blob; every other field is the full blob's
        want = {n: getattr(hf, n) for n, _ in hf._fields_ if n not in ("init_feature_search_region", "reserved")}
        want.update(omitted_sections=ALL & ~sections, bytes=hp.bytes,
                    **{n: getattr(hp, n) for n in ("off_cov", "off_selection", "off_traj", "off_partial", "off_patches")})
        if not sections & TRAJ:
            want.update(traj_count=0, traj_first=hf.traj_total)
        if not sections & PATCHES:
            want.update(n_patches=0)
        got = {n: getattr(hp, n) for n in want}
        assert got == want, i
        assert list(hp.init_feature_search_region) == list(hf.init_feature_search_region) and not any(hp.reserved)
        assert hp.bytes == 256 + sum(len(v) for v in sp.values())
        d = decode_snapshot(blobs[i])      # the Python decoder honours omitted_sections
        assert len(d["features"]) == (hf.n_features if sections & FEATURES else 0)
        assert len(d["selection"]) == (hf.n_selected if sections & SELECTION else 0)
        assert len(d["partial"]) == (hf.n_partial if sections & PARTIAL else 0) and len(d["patches"]) == hp.n_patches
        assert len(d["trajectory"]) == hp.traj_count and np.array_equal(d["xv"], decode_snapshot(full[i])["xv"])
        assert all((f["Pxy"] is None) == (not sections & COV) for f in d["features"])


def test_refusals_queue_nothing(five):
    e = five
    before = [single_raw(e, b) for b in range(5)]
    L = e.L
    for sections in (COV, COV | TRAJ, ALL & ~FEATURES):      # the covariance records cannot be walked without state_size
        rc, buf, offs = batch_call(e, 0, 5, sections)
        assert rc == _lib.SL2_ERR_INVALID and (buf == SENTINEL).all() and (offs == 2 ** 64 - 1).all()
    buf = np.full(4096, SENTINEL, dtype=np.uint8)
    o = np.full(8, 7, dtype=np.uint64)
    pb, po = buf.ctypes.data_as(_lib.vp), o.ctypes.data_as(_lib.vp)
    neg = np.array([[0, 0], [-1, 0]], dtype=np.int32)
    calls = [(e.h, -1, 1, ALL, None, pb, 4096, po, 0), (e.h, 0, 0, ALL, None, pb, 4096, po, 0), (e.h, 0, 6, ALL, None, pb, 4096, po, 0),
             (e.h, 4, 2, ALL, None, pb, 4096, po, 0), (e.h, 0, 1, ALL, None, None, 4096, po, 0), (e.h, 0, 1, ALL, None, pb, 4096, None, 0),
             (e.h, 0, 2, ALL, neg.ctypes.data_as(_lib.vp), pb, 4096, po, 0), (e.h, 0, 1, 64, None, pb, 4096, po, 0),
             (e.h, 0, 1, ALL | 128, None, pb, 4096, po, 0), (e.h, 0, 1, -1, None, pb, 4096, po, 0)]
    for args in calls:
        assert L.sl2_snapshot_batch(*args) == _lib.SL2_ERR_INVALID, args[1:4]
    assert (buf == SENTINEL).all() and (o == 7).all()
    assert [single_raw(e, b) for b in range(5)] == before


def test_device_form_and_its_capacity_check(five):
    """out, offsets and cursors in device memory: the bytes of the host form.  Told 16 bytes less than the total, the pack kernel
    writes no blob and the offsets are filled all the same."""
    e = five
    for sections in (ALL, FEATURES | SELECTION):
        rc, hbuf, hoffs = batch_call(e, 0, 5, sections, CURSORS5)
        assert rc == _lib.SL2_OK
        total = int(hoffs[5])
        room = e.snapshot_bound(sections) * 5      # (holds the blobs under any cursors)
        assert room >= total + 256
        d_out, d_off, d_cur = _lib.DeviceBuffer(room), _lib.DeviceBuffer(8 * 6), _lib.DeviceBuffer(8 * 5)
        d_cur.upload(np.array(CURSORS5, dtype=np.int32))
        for told in (total, total - 16):
            d_out.upload(np.full(room, SENTINEL, dtype=np.uint8))
            d_off.upload(np.full(6, 2 ** 64 - 1, dtype=np.uint64))
            assert e.snapshot_batch_device(d_out.ptr, told, d_off.ptr, 0, 5, sections, d_cur.ptr) == (d_out.ptr, d_off.ptr)
            e.synchronize()
            got, offs = d_out.download((room,), np.uint8), d_off.download((6,), np.uint64)
            assert np.array_equal(offs, hoffs)
            if told == total:
                assert np.array_equal(got[:total], hbuf[:total]) and (got[total:] == SENTINEL).all()
            else:
                assert (got == SENTINEL).all()
        # a negative cursor cannot be refused on the device: it is taken as 0
        d_cur.upload(np.array([[-5, 0]] * 5, dtype=np.int32))
        d_out.upload(np.full(room, SENTINEL, dtype=np.uint8))
        e.snapshot_batch_device(d_out.ptr, room, d_off.ptr, 0, 5, sections, d_cur.ptr)
        e.synchronize()
        rc, zbuf, zoffs = batch_call(e, 0, 5, sections, None)
        assert np.array_equal(d_off.download((6,), np.uint64), zoffs)
        assert np.array_equal(d_out.download((room,), np.uint8)[:int(zoffs[5])], zbuf[:int(zoffs[5])])
        # a misaligned device `out` is refused
        assert e.L.sl2_snapshot_batch(e.h, 0, 5, sections, None, _lib.vp(d_out.ptr + 8), room - 8, _lib.vp(d_off.ptr), 1) == _lib.SL2_ERR_INVALID
        for d in (d_out, d_off, d_cur):
            d.free()


def test_host_capacity_refusal_leaves_out_and_the_engine_alone():
    """SL2_ERR_CAPACITY: offsets[nseq] is the size to come back with, out is untouched, a second call with that size succeeds -
    and the engine goes on bit for bit like a twin that never made any of these calls."""
    pr = Pair(8, 4, batch=3, make_engine=False)
    e, twin = pr.make_engine_for(0, 3, 8), pr.make_engine_for(0, 3, 8)
    for k in range(2):
        for q in (e, twin):
            q.go_one_step(pr.frame_batch(k), save_trajectory=True)
    rc, buf, offs = batch_call(e, 0, 3, ALL)
    assert rc == _lib.SL2_OK
    total = int(offs[3])
    rc, small, offs2 = batch_call(e, 0, 3, ALL, out_bytes=total - 16)
    assert rc == _lib.SL2_ERR_CAPACITY and np.array_equal(offs2, offs) and (small == SENTINEL).all()
    rc, exact, offs3 = batch_call(e, 0, 3, ALL, out_bytes=total)
    assert rc == _lib.SL2_OK and np.array_equal(offs3, offs) and np.array_equal(exact[:total], buf[:total])
    assert (exact[total:] == SENTINEL).all()
    for k in range(2, 4):
        for q in (e, twin):
            q.go_one_step(pr.frame_batch(k), save_trajectory=True)
    for b in range(3):
        assert single_raw(e, b) == single_raw(twin, b), b
    assert_identity(e, 0, 3)


# ------------------------------------------------------------------------------------------------- shapes
def test_more_than_one_ballot_round():
    """66 known features in 70 slots: the counting phases walk the slots in two rounds of 64; deletions on both sides of the seam."""
    pr = Pair(66, 2, batch=3, max_features=70, n_select=12)
    e = pr.engine
    for k in range(2):
        e.go_one_step(pr.frame_batch(k), save_trajectory=True)
    assert_identity(e, 0, 3)
    assert e.delete_features([5, -1, 64]).tolist() == [True, False, True] and e.delete_features([65, 63, -1]).tolist() == [True, True, False]
    blobs, _ = assert_identity(e, 0, 3, [(0, 0), (1, 60), (0, 64)])
    assert [header(b).n_features for b in blobs] == [64, 65, 65] and [header(b).n_patches for b in blobs] == [64, 5, 1]
    assert_identity(e, 1, 2)


def test_across_the_scans_chunk():
    """Batch = the scan's chunk + 4 with maps of unequal size: the carry from the first chunk into the second, and ranges the
    four sequences of a sizing workgroup do not divide."""
    pr = Pair(6, 1, batch=1, make_engine=False)
    B = SCAN_CHUNK + 4
    spec, tpl = pr.specs[0], pr.templates[0]
    e = Engine(pr.cam, pr.params, B, 8)
    e.set_vehicle_state(np.tile(spec.xv0, (B, 1)), np.tile(spec.Pxx0, (B, 1, 1)))
    def add(seq0, nseq, first, n):
        e.add_known_features(np.tile(spec.feat_y[first:first + n], (nseq, 1, 1)), np.tile(spec.poses[0], (nseq, n, 1)),
                             np.tile(tpl[first:first + n], (nseq, 1, 1, 1)), seq0=seq0)
    add(0, B, 0, 3)
    add(100, 100, 3, 2)                            # sequences 100 .. 199: five features
    add(SCAN_CHUNK - 1, 3, 3, 3)                   # 255, 256, 257: six
    e.go_one_step(np.tile(pr.frames[0][0], (B, 1, 1)), save_trajectory=True)
    rc, buf, offs = batch_call(e, 0, B, ALL)
    assert rc == _lib.SL2_OK
    blobs = check_packing(buf, offs, B)
    assert (np.diff(offs.astype(np.int64)) > 0).all()
    assert [header(blobs[i]).n_features for i in (0, 150, SCAN_CHUNK - 1, SCAN_CHUNK, B - 1)] == [3, 5, 6, 6, 3]
    for b in (0, SCAN_CHUNK - 1, SCAN_CHUNK, B - 1):
        assert blobs[b] == single_raw(e, b), b
    assert all(header(blobs[b]).seq == b for b in range(B))
    assert_identity(e, 98, 5)
    assert_identity(e, SCAN_CHUNK - 4, 7)
    # the sections a publisher takes, over the whole batch: the same features and selection as the full blobs carry
    rc, sbuf, soffs = batch_call(e, 0, B, FEATURES | SELECTION)
    assert rc == _lib.SL2_OK
    small = check_packing(sbuf, soffs, B)
    for b in (1, SCAN_CHUNK + 1):
        assert section_bytes(small[b])["features"] == section_bytes(blobs[b])["features"]
        assert section_bytes(small[b])["selection"] == section_bytes(blobs[b])["selection"]
    e.close()


# ------------------------------------------------------------------------------------------------- graphs, groups, Python
def test_between_replayed_steps_of_a_captured_graph():
    """set_graph_mode(1), device frames in two alternating buffers (frames 0, 1 capture, 2 .. 5 replay): a batch snapshot after
    every step is the per-sequence snapshots, costs no capture, and the run is the run of an engine that made no snapshot call."""
    T = _lib.load_testing()
    pr = Pair(12, 6, batch=2, n_select=6, make_engine=False)
    engines = [pr.make_engine_for(0, 2, 12) for _ in range(2)]
    for e in engines:
        e.set_graph_mode(True)
    fb = pr.cam["width"] * pr.cam["height"]
    bufs = [_lib.DeviceBuffer(2 * fb) for _ in range(2)]
    cursors = [(0, 0), (0, 0)]
    for k in range(6):
        buf = bufs[k & 1]
        buf.upload(np.ascontiguousarray(pr.frame_batch(k), dtype=np.uint8))
        for e in engines:
            e.go_one_step(buf.ptr, on_device=True, seq_stride=fb, save_trajectory=True)
        rc, out, offs = batch_call(engines[0], 0, 2, ALL, cursors)       # queued behind the step, no wait in between
        assert rc == _lib.SL2_OK
        blobs = check_packing(out, offs, 2)
        for b in range(2):
            assert blobs[b] == single_raw(engines[0], b, *cursors[b]) and header(blobs[b]).steps_done == k + 1
        cursors = [(header(b).traj_total, header(b).next_free_label) for b in blobs]
        for e in engines:
            e.synchronize()
        assert T.sl2_debug_graph_captures(engines[0].h) == T.sl2_debug_graph_captures(engines[1].h) == min(k + 1, 2)
    for b in range(2):
        assert single_raw(engines[0], b) == single_raw(engines[1], b)
    for d in bufs:
        d.free()


def test_with_sequence_groups():
    pr = Pair(10, 3, batch=4, n_select=6, make_engine=False)
    e, plain = pr.make_engine_for(0, 4, 10), pr.make_engine_for(0, 4, 10)
    e.set_groups(2)
    for k in range(3):
        for q in (e, plain):
            q.go_one_step(pr.frame_batch(k), save_trajectory=True)
        blobs, _ = assert_identity(e, 0, 4)      # the first call is queued straight behind the step: the groups' streams have joined
        assert_identity(e, 1, 3, [(1, 0), (0, 4), (2, INT32_MAX)])
    for b in range(4):
        assert blobs[b] == single_raw(plain, b)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, C.Structure):
        return bytes(a) == bytes(b)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def test_python_snapshot_batch_returns_the_dicts_of_snapshot(five):
    e = five
    snaps, offs = e.snapshot_batch(0, 5, cursors=CURSORS5)
    assert len(snaps) == 5 and offs.dtype == np.uint64 and len(offs) == 6 and int(offs[0]) == 0
    for b in range(5):
        one = e.snapshot(b, *CURSORS5[b])
        assert _same(snaps[b], one), b
        assert int(offs[b + 1] - offs[b]) == (one["header"].bytes + 15) & ~15
    part, _ = e.snapshot_batch(1, 2, sections=FEATURES | SELECTION)
    for i, s in enumerate(part):
        one = e.snapshot(1 + i)
        assert [f["label"] for f in s["features"]] == [f["label"] for f in one["features"]]
        assert all(bytes(f["info"]) == bytes(g["info"]) and f["Pxy"] is None for f, g in zip(s["features"], one["features"]))
        assert np.array_equal(s["selection"], one["selection"]) and not s["patches"] and not s["partial"] and len(s["trajectory"]) == 0
    raw, roffs = e.snapshot_batch_raw()
    assert len(raw) == int(roffs[5]) and np.array_equal(roffs, e.snapshot_batch()[1])
