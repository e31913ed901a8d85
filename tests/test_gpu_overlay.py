"""Annotated frames on the device (include/scenelib2_amd.h, "annotated frames").

The rasteriser: the cases of overlay_cases.py through sl2_draw_items_batch, several images a launch, in every residency of
lists, frames and output and with strides above the minimum - all byte-equal to sl2_draw_items_host (which
tests/test_overlay_host.py holds to a NumPy restatement of the header's rules).

The engine form: a NumPy list builder that works ONLY from public accessors (sl2_get_features, sl2_get_vehicle_state,
sl2_get_cameras, sl2_get_partial_feature, sl2_get_feature_patch, the snapshot header's boxes) and takes the current projection
from the oracle's measurement model.  Where no coordinate that gets rounded lies within 1e-6 of a half-integer - asserted - the
list of sl2_overlay_items equals the builder's exactly, ints and doubles alike, and sl2_draw_overlays equals the builder's list
put through the host form."""
import numpy as np
import pytest

import display_helpers as dh
import oracle_api as oa
import overlay_cases as oc
from display_helpers import SENTINEL, assert_images, assert_lists_equal
from mapping_helpers import make_mapping_sequence
from scenelib2_amd import Engine, _lib, overlay
from slam_helpers import Pair

pytestmark = pytest.mark.gpu

SR, DESC, INIT = overlay.SL2_OVERLAY_SEARCH_REGIONS, overlay.SL2_OVERLAY_DESCRIPTORS, overlay.SL2_OVERLAY_INITIALISATION


# ------------------------------------------------------------------------------------------------- the rasteriser
def _groups():
    """The cases of one image size that share a patch array, as one batch each: {(w, h): (names, frames, lists, patches)}."""
    out = {}
    for name, (w, h), items, patches in oc.CASES:
        if patches is None and any(int(it["kind"]) == oc.PATCH for it in items):
            continue          # (a patch without an array draws nothing: it cannot share a launch that has one; see below)
        g = out.setdefault((w, h), dict(names=[], frames=[], lists=[], patches=None))
        g["names"].append(name)
        g["frames"].append(oc.frame_of(w, h, seed=len(name)))
        g["lists"].append(oc.items_array(items))
        if patches is not None:
            g["patches"] = patches
    return out


@pytest.fixture(scope="module")
def batches():
    groups = _groups()
    for (w, h), g in groups.items():
        g["want"] = np.stack([overlay.draw_items_host(f, l, g["patches"]) for f, l in zip(g["frames"], g["lists"])])
        g["frames"] = np.stack(g["frames"])
    return groups


def _draw(g, w, h, *residency, **pads):
    """(A host-resident list with a bad item is refused, tests/test_overlay_host.py: the bad_ cases go by device lists.)"""
    return dh.draw_items_batch(g, w, h, *residency, filler=oc.circle(w // 2, h // 2, 4, oc.GREEN), refused_prefix="bad_", **pads)


@pytest.mark.parametrize("size", oc.SIZES)
@pytest.mark.parametrize("residency", ["host", "device", "frames_on_device", "lists_and_out_on_device"])
def test_raster_cases_equal_the_host_form(batches, size, residency):
    w, h = size
    g = batches[size]
    fd, idv, od = dict(host=(0, 0, 0), device=(1, 1, 1), frames_on_device=(1, 0, 0), lists_and_out_on_device=(0, 1, 1))[residency]
    assert_images(_draw(g, w, h, fd, idv, od))


@pytest.mark.parametrize("size", oc.SIZES)
@pytest.mark.parametrize("pads", [(13, 3, 7), (4, 1, 4), (1, 0, 2)])
def test_strides_above_the_minimum(batches, size, pads):
    """seq_stride, item_stride and out_stride above their minima, device and host forms: an out_stride that keeps the rows
    4-byte aligned at width 64 (the dword stores) and ones that do not; nothing between the images is written."""
    w, h = size
    g = batches[size]
    for res in ((1, 1, 1), (0, 0, 0)):
        assert_images(_draw(g, w, h, *res, seq_pad=pads[0], item_pad=pads[1], out_pad=pads[2]))


def test_patch_without_an_array_and_single_image():
    for name, (w, h), items, patches in oc.CASES:
        if not name.startswith("patch_without_array"):
            continue
        f = oc.frame_of(w, h, 3)
        arr = oc.items_array(items)
        with pytest.raises(_lib.Sl2Error, match="patch index"):          # in a host-resident list the patch is refused ...
            overlay.draw_items(f[None], [arr], None)
        d_items, d_counts = _lib.DeviceBuffer(arr.nbytes), _lib.DeviceBuffer(4)          # ... in a device-resident one it draws nothing
        d_items.upload(arr)
        d_counts.upload(np.array([arr.size], np.int32))
        got = np.zeros((h, w, 3), np.uint8)
        vp = _lib.vp
        _lib.check(_lib.load().sl2_draw_items_batch(0, None, vp(f.ctypes.data), 0, 1, w, h, w * h, vp(d_items.ptr), arr.size, vp(d_counts.ptr), 1, None, 0, 0,
                                                    vp(got.ctypes.data), 3 * w * h, 0))
        assert np.array_equal(got, overlay.draw_items_host(f, arr, None)), name
        ring_only = overlay.draw_items(f[None], [arr[arr["kind"] == oc.RING]], None)          # the Python wrapper, one image, no patches
        assert np.array_equal(ring_only[0], got)
        d_items.free()
        d_counts.free()


def test_a_device_list_with_a_bad_count_or_item_is_clamped_and_skipped():
    """What the host would refuse, resident on the device: counts below 0 and above item_stride, a bad kind, a bad patch index."""
    L = _lib.load()
    w, h, n, stride = 70, 37, 4, 3
    f = np.stack([oc.frame_of(w, h, k) for k in range(n)])
    P = oc.patches_of(2)
    good = [oc.circle(30, 18, 7, oc.RED), oc.patch(40, 20, 1, oc.BLUE), oc.rect(3, 3, 60, 30, oc.GREEN)]
    items = np.zeros((n, stride), oc.ITEM)
    items[:] = oc.items_array(good)
    items[2, 0]["kind"] = 7
    items[2, 1]["patch"] = 2
    counts = np.array([-5, 1000, 3, 2], np.int32)
    want = [[], good, good[2:], good[:2]]
    bufs = [_lib.DeviceBuffer(a.nbytes) for a in (f, items, counts, P)]
    for b, a in zip(bufs, (f, items, counts, P)):
        b.upload(a)
    out = np.zeros((n, h, w, 3), np.uint8)
    vp = _lib.vp
    _lib.check(L.sl2_draw_items_batch(0, None, vp(bufs[0].ptr), 1, n, w, h, w * h, vp(bufs[1].ptr), stride, vp(bufs[2].ptr), 1, vp(bufs[3].ptr), 121, 2,
                                      out.ctypes.data_as(vp), 3 * w * h, 0), L)
    for i in range(n):
        assert np.array_equal(out[i], overlay.draw_items_host(f[i], oc.items_array(want[i]), P)), i
    for b in bufs:
        b.free()


# ------------------------------------------------------------------------------------------------- the engine form
def _rnd(v):
    """int(v + 0.5) by C truncation, or None where the item is omitted."""
    if not np.isfinite(v) or not -40000.0 < v < 40000.0:
        return None
    c = int(v + 0.5)
    return c if -32767 <= c <= 32767 else None


def _zeroed_z(xp, y):
    """Third component of R(q)^T (y - r): only its sign is used."""
    w, x, yy, z = xp[3:7]
    R = np.array([[1 - 2 * (yy * yy + z * z), 2 * (x * yy - w * z), 2 * (x * z + w * yy)],
                  [2 * (x * yy + w * z), 1 - 2 * (x * x + z * z), 2 * (yy * z - w * x)],
                  [2 * (x * z - w * yy), 2 * (yy * z + w * x), 1 - 2 * (x * x + yy * yy)]])
    return float((R.T @ (np.asarray(y) - xp[:3]))[2])


def _colour(marked, selected, matched):
    return oc.GREEN if marked else oc.RED if selected and matched else oc.BLUE if selected else oc.YELLOW


def build_list(e, seq, i, layers, marked=-1):
    """The draw list of sequence `seq` (list i of a call) from public accessors: (items, rounded) - rounded = every coordinate
    that went through the rounding."""
    N = e.max_features
    xv, _ = e.get_vehicle_state(seq, 1)
    xp = xv[0, :7]
    cam = e.get_cameras(seq, 1)[0]
    partial = {pf["label"]: pf for pf in e.partial_features(seq)}
    items, rounded = [], []
    for k, f in enumerate(e.features(seq)):
        mark = f["label"] == marked
        if f["fully_initialised"]:
            if not _zeroed_z(xp, f["y"]) > 0:
                continue
            hi = oa.measurement_model(cam, xp, f["y"])["h"]
            sel, ok = f["selected"], f["success"]
            rgb = _colour(mark, sel, ok)
            if (layers & SR) and sel:
                rounded += [f["h"][0], f["h"][1]]
                c = (_rnd(f["h"][0]), _rnd(f["h"][1]))
                if None not in c:
                    S = f["S"]
                    items.append(oc.ring(c[0], c[1], S[1, 1], -(S[0, 1] + S[1, 0]), S[0, 0], 9.0 * (S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]), rgb, f["label"]))
            if layers & DESC:
                p = f["z"] if sel and ok else hi
                rounded += [p[0], p[1]]
                c = (_rnd(p[0]), _rnd(p[1]))
                if None not in c:
                    items.append(oc.patch(c[0], c[1], i * N + k, rgb, f["label"]))
        elif layers & SR:
            pf = partial[f["label"]]
            for k2 in oc.particles_drawn(pf["n_particles"]):
                p = pf["particles"][k2]
                rounded += [p[3], p[4]]
                c = (_rnd(p[3]), _rnd(p[4]))
                if None not in c:
                    items.append(oc.ring(c[0], c[1], p[7], 2.0 * p[8], p[9], 9.0, oc.GREEN if mark else oc.YELLOW, f["label"]))
    if layers & INIT:
        hd = e.snapshot(seq)["header"]
        if hd.location_selected_flag:
            items.append(oc.rect(hd.uu - 6, hd.vv - 6, hd.uu + 6, hd.vv + 6, oc.GREEN))
        if hd.init_feature_search_region_defined_flag:
            items.append(oc.rect(*hd.init_feature_search_region, oc.GREEN))
    return oc.items_array(items), rounded


def patch_array(e, seq0, nseq):
    """patches [nseq * max_features][121] as the header describes them: entry i * max_features + k = the template of feature k."""
    N = e.max_features
    P = np.zeros((nseq * N, 121), np.uint8)
    for i in range(nseq):
        for k, f in enumerate(e.features(seq0 + i)):
            P[i * N + k] = e.feature_patch(seq0 + i, f["label"]).reshape(-1)
    return P


def assert_clear_of_half_integers(rounded):
    v = np.asarray(rounded, np.float64)
    v = v[np.isfinite(v)]
    assert (np.abs(v - np.floor(v) - 0.5) > 1e-6).all(), "a rounded coordinate lies within 1e-6 of a half-integer: choose another seed"


def check_engine(e, frames, seq0, nseq, layers, marked=None, rounded_out=None):
    """sl2_overlay_items against the builder, sl2_draw_overlays against the builder's lists put through the host form."""
    lists = e.overlay_items(seq0, nseq, layers, marked)
    P = patch_array(e, seq0, nseq)
    imgs = e.draw_overlays(frames[seq0:seq0 + nseq], seq0, nseq, layers, marked)
    built = []
    for i in range(nseq):
        want, rounded = build_list(e, seq0 + i, i, layers, -1 if marked is None else int(marked[i]))
        assert_clear_of_half_integers(rounded)
        if rounded_out is not None:
            rounded_out += rounded
        assert_lists_equal(lists[i], want, "sequence %d, layers %d" % (seq0 + i, layers))
        assert want.size <= e.overlay_item_bound()
        host = overlay.draw_items_host(frames[seq0 + i], want, P)
        assert np.array_equal(imgs[i], host), (seq0 + i, layers, np.argwhere((imgs[i] != host).any(axis=2))[:5].tolist())
        built.append(want)
    return built, imgs


SEED = 7


@pytest.fixture(scope="module")
def scene():
    """Batch 3, the shipped 320 x 240 camera, a dozen known features plus mapping, until a partially initialised feature, a
    conversion, a failed match and a deletion have all occurred (asserted).  Sequence 1 has one feature deleted by hand on the
    way, sequence 2 sits out some steps: the three lists differ."""
    cam, params, spec, frames, templates = make_mapping_sequence(seed=SEED, n_known=12, n_frames=60)
    assert (cam["width"], cam["height"]) == (320, 240)
    B = 3
    e = Engine(cam, params, B, 24)
    e.set_vehicle_state(np.tile(spec.xv0, (B, 1)), np.tile(spec.Pxx0, (B, 1, 1)))
    e.add_known_features(np.tile(spec.feat_y, (B, 1, 1)), np.tile(spec.xp_org(), (B, 1, 1)), np.tile(templates, (B, 1, 1, 1)))
    seen = dict(partial=False, conversion=False, failed=False, deletion=False, particles=False)
    last = 0
    for k in range(1, 60):
        if k == 5:
            e.set_active([1, 1, 0])
        if k == 9:
            e.set_active([1, 1, 1])
        if k == 6:
            victim = [f["label"] for f in e.features(1) if f["fully_initialised"]][2]
            seen["deletion"] = bool(e.delete_features([-1, victim, -1])[1])
        e.go_one_step(np.tile(frames[k], (B, 1, 1)), save_trajectory=True, enable_mapping=True)
        last = k
        info = e.partial_feature(0)
        seen["conversion"] |= info["info"]["converted"] > 0
        seen["partial"] = info["pf"] is not None
        seen["particles"] = info["pf"] is not None and bool(np.any(info["pf"]["particles"][:, 7] > 0))
        if k >= 12 and seen["partial"] and seen["particles"] and seen["conversion"] and seen["deletion"]:
            break
    # the failed match: sequence 2 alone steps once more, on a frame without texture - its selected features stay unmatched
    e.set_active([0, 0, 1])
    shown = np.tile(frames[last], (B, 1, 1))
    shown[2] = 128
    e.go_one_step(shown, save_trajectory=True, enable_mapping=True)
    e.set_active([1, 1, 1])
    seen["failed"] = any(f["selected"] and not f["success"] for f in e.features(2))
    print("overlay scene after %d steps: %s; features %s" % (last, seen, [len(e.features(b)) for b in range(B)]))
    assert all(seen.values()), seen          # ... and a partial feature whose particles were searched is in flight right now
    yield dict(e=e, frames=shown, cam=cam)
    e.close()


def test_scene_holds_every_kind_of_item(scene):
    e = scene["e"]
    rounded = []
    built, imgs = check_engine(e, scene["frames"], 0, 3, overlay.SL2_OVERLAY_ALL, rounded_out=rounded)
    kinds = np.concatenate([b["kind"] for b in built])
    colours = {tuple(c) for b in built for c in b["rgb"].tolist()}
    assert {oc.RING, oc.PATCH}.issubset(set(kinds.tolist())) and len(rounded) > 20
    assert oc.RED in colours and oc.YELLOW in colours and oc.BLUE in colours
    # a string of particle ellipses: several yellow rings that carry one label, along the ray
    labels, n = np.unique(built[0]["label"][(built[0]["kind"] == oc.RING) & (built[0]["rgb"] == oc.YELLOW).all(axis=1)], return_counts=True)
    assert n.size and n.max() >= 5
    assert not np.array_equal(built[0], built[1])          # the sequences differ: sequence 1 lost a feature
    for i in range(3):          # something was drawn, in colour
        assert (imgs[i][:, :, 0] != imgs[i][:, :, 2]).any()


@pytest.mark.parametrize("layers", range(8))
def test_every_subset_of_the_layers(scene, layers):
    built, _ = check_engine(scene["e"], scene["frames"], 0, 3, layers)
    if layers == 0:
        assert all(b.size == 0 for b in built)
    if not layers & DESC:
        assert all(not (b["kind"] == oc.PATCH).any() for b in built)
    if not layers & SR:
        assert all(not (b["kind"] == oc.RING).any() for b in built)
    if not layers & INIT:
        assert all(not (b["kind"] == oc.RECT).any() for b in built)


def test_marked_labels_null_and_a_range_that_starts_late(scene):
    e = scene["e"]
    partial_label = e.partial_feature(0)["pf"]["label"]
    full_label = [f["label"] for f in e.features(1) if f["fully_initialised"]][0]
    marked = np.array([partial_label, full_label, -1], np.int32)
    built, _ = check_engine(e, scene["frames"], 0, 3, overlay.SL2_OVERLAY_ALL, marked)
    for b, lab in zip(built[:2], marked[:2]):
        assert (b["rgb"][b["label"] == lab] == oc.GREEN).all() and (b["label"] == lab).any()
    plain, _ = check_engine(e, scene["frames"], 0, 3, overlay.SL2_OVERLAY_ALL, None)
    assert not np.array_equal(plain[0]["rgb"], built[0]["rgb"]) and np.array_equal(plain[2], built[2])
    # seq0 > 0: list 0 of the call is sequence 1, and the patch indices count from the call's first sequence
    late, _ = check_engine(e, scene["frames"], 1, 2, overlay.SL2_OVERLAY_ALL, marked[1:])
    shifted = built[1].copy()
    shifted["patch"][shifted["kind"] == oc.PATCH] -= e.max_features
    assert_lists_equal(late[0], shifted, "seq0 = 1")
    assert 0 <= late[0]["patch"].max() < e.max_features


@pytest.fixture(scope="module")
def large_map():
    for e, state, cam in dh.large_map():
        yield dict(e=e, cam=cam)


def test_large_map_two_rounds_of_slots_the_patches_count_on(large_map):
    """70 fully initialised features in front of the camera, one sequence: the second round of 64 slots has 6 live lanes, and its
    patches are numbered on from the 64 live features of the first.  The drawing equals the host form on the device's own list."""
    e, cam = large_map["e"], large_map["cam"]
    frames = oc.frame_of(cam["width"], cam["height"], seed=5)[None]
    marked = np.array([66], np.int32)
    built, imgs = check_engine(e, frames, 0, 1, overlay.SL2_OVERLAY_ALL, marked)
    b = built[0]
    assert b["kind"].tolist() == [oc.PATCH] * 70          # (never stepped: nothing is selected, no search region)
    assert b["patch"].tolist() == list(range(70)) and b["label"].tolist() == list(range(70))          # slot order across the two rounds
    assert tuple(b[66]["rgb"]) == oc.GREEN and tuple(b[65]["rgb"]) == oc.YELLOW
    own = e.overlay_items(0, 1, overlay.SL2_OVERLAY_ALL, marked)[0]
    assert np.array_equal(imgs[0], overlay.draw_items_host(frames[0], own, patch_array(e, 0, 1)))


def test_device_forms_equal_the_host_forms(scene):
    """sl2_overlay_items and sl2_draw_overlays with everything in device memory, strides above the minimum."""
    e, frames = scene["e"], scene["frames"]
    B, W, H = 3, 320, 240
    stride = e.overlay_item_bound() + 5
    d_items, d_counts = _lib.DeviceBuffer(64 * stride * B), _lib.DeviceBuffer(4 * B)
    marked = np.array([-1, 3, 0], np.int32)
    d_marked = _lib.DeviceBuffer(4 * B)
    d_marked.upload(marked)
    vp = _lib.vp
    _lib.check(e.L.sl2_overlay_items(e.h, 0, B, 7, vp(d_marked.ptr), vp(d_items.ptr), stride, vp(d_counts.ptr), 1), e.L)
    e.synchronize()
    counts = d_counts.download((B,), np.int32)
    items = d_items.download((B, stride), oc.ITEM)
    want = e.overlay_items(0, B, 7, marked)
    for i in range(B):
        assert counts[i] == want[i].size and items[i, :counts[i]].tobytes() == want[i].tobytes(), i
    seq_stride, out_stride = W * H + 64, 3 * W * H + 36
    padded = np.zeros((B, seq_stride), np.uint8)
    padded[:, :W * H] = frames.reshape(B, -1)
    d_frames, d_out = _lib.DeviceBuffer(padded.nbytes), _lib.DeviceBuffer(B * out_stride)
    d_frames.upload(padded)
    d_out.upload(np.full(B * out_stride, SENTINEL, np.uint8))
    e.draw_overlays_device(d_frames.ptr, d_out.ptr, 0, B, 7, d_marked.ptr, seq_stride, out_stride)
    e.synchronize()
    out = d_out.download((B, out_stride), np.uint8)
    host = e.draw_overlays(frames, 0, B, 7, marked)
    assert np.array_equal(out[:, :3 * W * H].reshape(B, H, W, 3), host) and (out[:, 3 * W * H:] == SENTINEL).all()
    # host output with a stride of its own, frames resident on the device
    strided = e.draw_overlays(d_frames.ptr, 0, B, 7, marked, on_device=True, seq_stride=seq_stride, out_stride=out_stride)
    assert np.array_equal(strided[:, :3 * W * H].reshape(B, H, W, 3), host) and not strided[:, 3 * W * H:].any()
    for d in (d_items, d_counts, d_marked, d_frames, d_out):
        d.free()


def test_host_frames_in_front_of_a_device_output_are_consumed_when_the_call_returns(scene):
    """frames_on_device = 0 with out_on_device = 1: the call waits until the (pageable) frames are copied, so the caller may
    overwrite them at once; the images are those of the host form."""
    e, frames = scene["e"], scene["frames"]
    B, W, H = 3, 320, 240
    want = e.draw_overlays(frames, 0, B, 7)
    d_out = _lib.DeviceBuffer(B * 3 * W * H)
    mine = frames.copy()
    vp = _lib.vp
    _lib.check(e.L.sl2_draw_overlays(e.h, 0, B, vp(mine.ctypes.data), W * H, 0, 7, None, vp(d_out.ptr), 3 * W * H, 1), e.L)
    mine[:] = 255                                    # (the buffer is the caller's again)
    e.synchronize()
    assert np.array_equal(d_out.download((B, H, W, 3), np.uint8), want)
    d_out.free()


def test_refusals_name_the_sequences(scene):
    e = scene["e"]
    L, vp = e.L, _lib.vp
    bound = e.overlay_item_bound()
    items, counts = np.zeros((3, bound), oc.ITEM), np.zeros(3, np.int32)
    ip, cp = vp(items.ctypes.data), vp(counts.ctypes.data)
    msg = lambda: L.sl2_last_error().decode()
    assert L.sl2_overlay_items(e.h, 2, 2, 7, None, ip, bound, cp, 0) == _lib.SL2_ERR_INVALID
    assert "sl2_overlay_items: sequences 2 .. 3" in msg() and "outside the batch" in msg()
    assert L.sl2_overlay_items(e.h, 1, 2, 7, None, ip, bound - 1, cp, 0) == _lib.SL2_ERR_INVALID
    assert "sequences 1 .. 2" in msg() and "item_stride" in msg()
    assert L.sl2_overlay_items(e.h, 0, 3, 8, None, ip, bound, cp, 0) == _lib.SL2_ERR_INVALID and "layers" in msg()
    f, out = scene["frames"], np.zeros((3, 3 * 320 * 240), np.uint8)
    fp, op = vp(f.ctypes.data), vp(out.ctypes.data)
    assert L.sl2_draw_overlays(e.h, 1, 3, fp, 76800, 0, 7, None, op, 230400, 0) == _lib.SL2_ERR_INVALID
    assert "sl2_draw_overlays: sequences 1 .. 3" in msg() and "outside the batch" in msg()
    assert L.sl2_draw_overlays(e.h, 1, 2, fp, 76800, 0, 7, None, op, 230399, 0) == _lib.SL2_ERR_INVALID
    assert "sequences 1 .. 2" in msg() and "out_stride" in msg()
    assert L.sl2_draw_overlays(e.h, 0, 3, None, 76800, 0, 7, None, op, 230400, 0) == _lib.SL2_ERR_INVALID and "null frames" in msg()
    assert not out.any() and not items["kind"].any()


def test_monoslam_draw_raw_ar_is_the_engine_call_with_the_check_boxes_in_the_reference_s_order():
    """MonoSLAM.DrawRawAR(frame, out, descriptors, search regions, initialisation): the argument order of the reference's three
    check boxes is not the order of the layer bits."""
    from scenelib2_amd import MonoSLAM
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=20)
    m = MonoSLAM(max_features=16).InitFromValues(cam, params, spec.xv0, spec.Pxx0)
    xo = spec.xp_org()
    for i in range(spec.n_features):
        m.AddNewKnownFeature(spec.feat_y[i], xo[i], templates[i])
    k = 0
    for k in range(1, 20):          # until a feature is being initialised: every layer has something to show
        m.GoOneStep(frames[k], enable_mapping=True)
        if k >= 6 and m._engine.partial_feature(0)["pf"] is not None:
            break
    m.marked_feature_label_ = 1
    eng, f = m._engine, frames[k][None]
    flags = {(d, s, i): (SR if s else 0) | (DESC if d else 0) | (INIT if i else 0) for d in (0, 1) for s in (0, 1) for i in (0, 1)}
    seen = set()
    for (d, s, i), layers in flags.items():
        out = np.zeros((cam["height"], cam["width"], 3), np.uint8)
        img = m.DrawRawAR(frames[k], out, bool(d), bool(s), bool(i))
        want = eng.draw_overlays(f, 0, 1, layers, [1])[0]
        assert np.array_equal(img, want) and np.array_equal(out, want), (d, s, i)
        seen.add(want.tobytes())
    assert len(seen) >= 4          # descriptors and search regions each change the picture
    assert np.array_equal(m.DrawRawAR(frames[k]), eng.draw_overlays(f, 0, 1, 7, [1])[0])
    assert (eng.draw_overlays(f, 0, 1, 7, [1])[0] == (0, 255, 0)).all(axis=2).any()          # the marked feature is green


def test_engine_refusals(scene):
    e = scene["e"]
    L, vp = e.L, _lib.vp
    bound = e.overlay_item_bound()
    items, counts = np.zeros((3, bound), oc.ITEM), np.zeros(3, np.int32)
    f, out = scene["frames"], np.zeros((3, 3 * 320 * 240), np.uint8)
    ip, cp, fp, op = (vp(a.ctypes.data) for a in (items, counts, f, out))
    for args in ((e.h, -1, 1, 7, None, ip, bound, cp, 0), (e.h, 0, 4, 7, None, ip, bound, cp, 0), (e.h, 3, 1, 7, None, ip, bound, cp, 0),
                 (e.h, 0, 0, 7, None, ip, bound, cp, 0), (e.h, 0, 3, 8, None, ip, bound, cp, 0), (e.h, 0, 3, 7, None, None, bound, cp, 0),
                 (e.h, 0, 3, 7, None, ip, bound, None, 0), (e.h, 0, 3, 7, None, ip, bound - 1, cp, 0)):
        assert L.sl2_overlay_items(*args) == _lib.SL2_ERR_INVALID, args[1:4]
    for args in ((e.h, 0, 4, fp, 76800, 0, 7, None, op, 230400, 0), (e.h, 2, 2, fp, 76800, 0, 7, None, op, 230400, 0),
                 (e.h, 0, 3, None, 76800, 0, 7, None, op, 230400, 0), (e.h, 0, 3, fp, 76800, 0, 7, None, None, 230400, 0),
                 (e.h, 0, 3, fp, 76799, 0, 7, None, op, 230400, 0), (e.h, 0, 3, fp, 76800, 0, 7, None, op, 230399, 0),
                 (e.h, 0, 3, fp, 76800, 0, 16, None, op, 230400, 0)):
        assert L.sl2_draw_overlays(*args) == _lib.SL2_ERR_INVALID, args[1:3]
    assert L.sl2_last_error().decode() == "sl2_draw_overlays: sequences 0 .. 2: layers with bits outside SL2_OVERLAY_ALL"
    assert not items["kind"].any() and not out.any()


def test_a_paused_sequence_is_still_drawn(scene):
    e = scene["e"]
    before = e.overlay_items()
    img = e.draw_overlays(scene["frames"])
    e.set_active([1, 0, 0])
    try:
        after, _ = check_engine(e, scene["frames"], 0, 3, overlay.SL2_OVERLAY_ALL)
        for a, b in zip(after, before):
            assert a.tobytes() == b.tobytes()
        assert np.array_equal(e.draw_overlays(scene["frames"]), img)
    finally:
        e.set_active([1, 1, 1])


def test_a_feature_behind_the_camera_vanishes(scene):
    """The camera of sequence 1 turned about its y axis through sl2_set_vehicle_state: every fully initialised feature lies behind
    it and yields nothing; the stored particle records and the boxes stay."""
    e = scene["e"]
    xv, Pxx = e.get_vehicle_state(1, 1)
    full = {f["label"] for f in e.features(1) if f["fully_initialised"]}
    before = e.overlay_items(1, 1)[0]
    assert np.isin(before["label"], list(full)).any()
    turned = xv.copy()
    w, x, y, z = xv[0, 3:7]
    turned[0, 3:7] = (-y, -z, w, x)          # q * (0, 0, 1, 0): half a turn about the camera's own y axis
    e.set_vehicle_state(turned, Pxx, seq0=1)
    try:
        built, _ = check_engine(e, scene["frames"], 0, 3, overlay.SL2_OVERLAY_ALL)
        assert not np.isin(built[1]["label"], list(full)).any()
        assert built[1].size == before.size - np.isin(before["label"], list(full)).sum()
    finally:
        e.set_vehicle_state(xv, Pxx, seq0=1)
    assert e.overlay_items(1, 1)[0].tobytes() == before.tobytes()


def test_with_sequence_groups():
    pr = Pair(10, 3, batch=4, n_select=6, make_engine=False)
    e, plain = pr.make_engine_for(0, 4, 10), pr.make_engine_for(0, 4, 10)
    e.set_groups(2)
    for k in range(3):
        for q in (e, plain):
            q.go_one_step(pr.frame_batch(k), save_trajectory=True)
        frames = np.ascontiguousarray(pr.frame_batch(k), dtype=np.uint8).reshape(4, pr.cam["height"], pr.cam["width"])
        built, imgs = check_engine(e, frames, 0, 4, overlay.SL2_OVERLAY_ALL)      # queued straight behind the step: the groups' streams have joined
        check_engine(e, frames, 1, 3, SR | DESC, np.array([0, 2, -1], np.int32))
    for b, w in zip(plain.overlay_items(), built):
        assert b.tobytes() == w.tobytes()
    assert np.array_equal(plain.draw_overlays(frames), imgs)
    for q in (e, plain):
        q.close()


def test_between_replayed_steps_of_a_captured_graph():
    """set_graph_mode(1), device frames in two alternating buffers: overlay calls in every form between the steps cost no
    capture, and the engine's state stays bit-identical to a twin that never draws."""
    T = _lib.load_testing()
    pr = Pair(12, 6, batch=2, n_select=6, make_engine=False)
    engines = [pr.make_engine_for(0, 2, 12) for _ in range(2)]
    for e in engines:
        e.set_graph_mode(True)
    W, H = pr.cam["width"], pr.cam["height"]
    fb = W * H
    bufs = [_lib.DeviceBuffer(2 * fb) for _ in range(2)]
    d_out = _lib.DeviceBuffer(2 * 3 * fb)
    for k in range(6):
        buf = bufs[k & 1]
        frames = np.ascontiguousarray(pr.frame_batch(k), dtype=np.uint8).reshape(2, H, W)
        buf.upload(frames)
        for e in engines:
            e.go_one_step(buf.ptr, on_device=True, seq_stride=fb, save_trajectory=True)
        e = engines[0]
        e.draw_overlays_device(buf.ptr, d_out.ptr)          # queued behind the step, no wait in between
        dev = d_out.download((2, H, W, 3), np.uint8)
        _, imgs = check_engine(e, frames, 0, 2, overlay.SL2_OVERLAY_ALL, np.array([k, -1], np.int32))
        assert np.array_equal(dev, e.draw_overlays(buf.ptr, on_device=True)) and imgs.shape == dev.shape
        for q in engines:
            q.synchronize()
        assert T.sl2_debug_graph_captures(engines[0].h) == T.sl2_debug_graph_captures(engines[1].h) == min(k + 1, 2)
    a, b = engines[0].save_sequences(0, 2), engines[1].save_sequences(0, 2)
    assert [bytes(x) for x in a] == [bytes(x) for x in b]
    for d in bufs + [d_out]:
        d.free()
    for e in engines:
        e.close()
