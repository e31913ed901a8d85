"""Host-side mirror of the reference's MonoSLAM / Kalman / Feature interface over the
C ABI (include/scenelib2_amd.h).

* `Engine` — the batched engine: B independent sequences stepped together.
* `MonoSLAM` — a single-sequence object with the reference's member names
  (scenelib2/monoslam.h:69-219): Init(cfg), GoOneStep(frame, save_trajectory,
  enable_mapping), xv_, Pxx_, feature_list_, selected_feature_list_,
  trajectory_store_, AddNewKnownFeature, print_robot_state ... so that tests read
  like the reference's own usage (examples/MonoSlamSceneLib1.cpp:132-142).

All numerical work happens in the HIP library; nothing here computes SLAM math.
"""
import ctypes as C

import os

import numpy as np

from . import _lib
from .config import load_config, read_pgm, resolve_identifier


def decode_snapshot(raw):
    """One snapshot blob (sl2_snapshot, or one blob of sl2_snapshot_batch; bytes-like, the blob at its start) as a dict of numpy
    arrays / python values.  A section the blob does not carry (header.omitted_sections) decodes as empty: no features, an empty
    selection ...; without SL2_SNAP_COV a feature's Pxy / Pyy are None."""
    h = _lib.sl2_snapshot_header.from_buffer_copy(raw[:256])
    assert h.magic == 0x53324C53 and 256 <= h.bytes <= len(raw)
    has = lambda bit: not (h.omitted_sections & bit)
    f64 = lambda off, n: np.frombuffer(raw, dtype=np.float64, count=n, offset=off).copy()
    out = dict(header=h, xv=f64(h.off_xv, 13), Pxx=f64(h.off_Pxx, 169).reshape(13, 13), features=[], partial=[], patches={})
    fsz = C.sizeof(_lib.sl2_feature_info)
    cov = h.off_cov
    for i in range(h.n_features if has(_lib.SL2_SNAP_FEATURES) else 0):
        f = _lib.sl2_feature_info.from_buffer_copy(raw[h.off_features + i * fsz: h.off_features + (i + 1) * fsz])
        d = f.state_size
        Pxy = Pyy = None
        if has(_lib.SL2_SNAP_COV):
            Pxy = f64(cov, 13 * d).reshape(13, d)
            Pyy = f64(cov + 13 * d * 8, d * d).reshape(d, d)
            cov += (13 * d + d * d) * 8
        out["features"].append(dict(info=f, label=f.label, Pxy=Pxy, Pyy=Pyy))
    n_sel = h.n_selected if has(_lib.SL2_SNAP_SELECTION) else 0
    out["selection"] = np.frombuffer(raw, dtype=np.int32, count=n_sel, offset=h.off_selection).copy()
    out["trajectory"] = f64(h.off_traj, 3 * h.traj_count).reshape(-1, 3)
    off = h.off_partial
    for _ in range(h.n_partial if has(_lib.SL2_SNAP_PARTIAL) else 0):
        pi = _lib.sl2_partial_info.from_buffer_copy(raw[off: off + 32])
        parts = f64(off + 32, 12 * pi.n_particles).reshape(-1, 12)
        out["partial"].append(dict(info=pi, particles=parts))
        off += 32 + 96 * pi.n_particles
    for k in range(h.n_patches):
        o = h.off_patches + 128 * k
        lab = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=o)[0])
        out["patches"][lab] = np.frombuffer(raw, dtype=np.uint8, count=121, offset=o + 4).reshape(11, 11).copy()
    return out


class Engine:
    """B independent MonoSLAM instances on one GPU (one HIP stream)."""

    def __init__(self, cam, params, batch, max_features, device=0, stream=None, lib=None):
        self.L = lib or _lib.load()          # lib = _lib.load_testing(): the TEST build (kernel variants, hooks)
        self.cam = dict(cam)
        self.params = dict(params)
        self.batch = int(batch)
        self.max_features = int(max_features)
        self.device = int(device)
        self.frame_bytes = int(cam["width"]) * int(cam["height"])
        self._cam = _lib.make_camera(cam)
        self._prm = _lib.make_params(params)
        h = _lib.vp()
        self._ck(self.L.sl2_create(C.byref(self._cam), C.byref(self._prm), self.batch, self.max_features,
                                     self.device, _lib.vp(stream) if stream else None, C.byref(h)))
        self.h = h

    def _ck(self, rc):
        _lib.check(rc, self.L)

    def close(self):
        if getattr(self, "h", None):
            self.L.sl2_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup -------------------------------------------------------------
    def set_vehicle_state(self, xv, Pxx, seq0=0):
        xv = np.ascontiguousarray(xv, dtype=np.float64).reshape(-1, 13)
        Pxx = np.ascontiguousarray(Pxx, dtype=np.float64).reshape(-1, 13, 13)
        assert xv.shape[0] == Pxx.shape[0]
        self._ck(self.L.sl2_set_vehicle_state(self.h, seq0, xv.shape[0], _lib.dp(xv), _lib.dp(Pxx)))

    def get_vehicle_state(self, seq0=0, nseq=None):
        nseq = self.batch - seq0 if nseq is None else nseq
        xv = np.zeros((nseq, 13))
        Pxx = np.zeros((nseq, 13, 13))
        self._ck(self.L.sl2_get_vehicle_state(self.h, seq0, nseq, _lib.dp(xv), _lib.dp(Pxx)))
        return xv, Pxx

    def add_known_features(self, y, xp_org, patches, seq0=0):
        """y [nseq][nfeat][3], xp_org [nseq][nfeat][7], patches [nseq][nfeat][11][11] uint8."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        nseq, nfeat = y.shape[0], y.shape[1]
        xp = np.ascontiguousarray(xp_org, dtype=np.float64).reshape(nseq, nfeat, 7)
        p = np.ascontiguousarray(patches, dtype=np.uint8).reshape(nseq, nfeat, 121)
        self._ck(self.L.sl2_add_known_features(self.h, seq0, nseq, nfeat, _lib.dp(y), _lib.dp(xp), _lib.u8p(p)))

    def set_feature_covariances(self, Pyy, seq0=0):
        """Pyy [nseq][nfeat][3][3]: prior covariance of the first nfeat features of each sequence."""
        P = np.ascontiguousarray(Pyy, dtype=np.float64)
        nseq, nfeat = P.shape[0], P.shape[1]
        self._ck(self.L.sl2_set_feature_covariances(self.h, seq0, nseq, nfeat, _lib.dp(P.reshape(nseq, nfeat, 9))))

    # ---- stepping ----------------------------------------------------------
    def _frames_arg(self, frames, seq_stride, on_device):
        if on_device:
            return _lib.vp(int(frames)), int(seq_stride if seq_stride else self.frame_bytes), 1, None
        f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(self.batch, self.frame_bytes)
        return f.ctypes.data_as(_lib.vp), self.frame_bytes, 0, f

    def go_one_step(self, frames, save_trajectory=False, enable_mapping=False, on_device=False, seq_stride=0):
        ptr, stride, dev, keep = self._frames_arg(frames, seq_stride, on_device)
        self._ck(self.L.sl2_go_one_step(self.h, ptr, stride, dev, int(save_trajectory), int(enable_mapping)))
        if keep is not None:
            self.synchronize()  # host buffer must outlive the async H2D copy

    def set_active(self, mask, seq0=0, on_device=False):
        """Which sequences take part in the steps issued from now on (sl2_set_active_sequences): mask[i] != 0 = sequence
        seq0 + i does.  A paused sequence is left exactly as it was by every step.  mask: array-like of len <= batch - seq0
        (consumed before the call returns), or with on_device=True a (device pointer, count) pair.  Never synchronises."""
        if on_device:
            ptr, n = mask
            self._ck(self.L.sl2_set_active_sequences(self.h, int(seq0), int(n), C.cast(_lib.vp(int(ptr)), _lib.c_u8p), 1))
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
        self._ck(self.L.sl2_set_active_sequences(self.h, int(seq0), int(m.size), _lib.u8p(m), 0))

    def active(self, seq0=0, nseq=None):
        """The mask as the steps queued so far leave it: uint8 [nseq] (sl2_get_active_sequences; synchronises)."""
        nseq = self.batch - seq0 if nseq is None else nseq
        out = np.zeros(nseq, dtype=np.uint8)
        self._ck(self.L.sl2_get_active_sequences(self.h, int(seq0), int(nseq), _lib.u8p(out)))
        return out

    def set_delta_t(self, dt, seq0=0, on_device=False):
        """The time step of sequences seq0, seq0 + 1, ... from their next predict on (sl2_set_delta_t); what they were owed is
        cleared.  dt: a scalar or array-like of len <= batch - seq0, every value finite and > 0 (consumed before the call
        returns), or with on_device=True a (device pointer, count) pair, whose invalid entries are skipped.  Never
        synchronises, drops no captured step, does not consult the mask."""
        if on_device:
            ptr, n = dt
            self._ck(self.L.sl2_set_delta_t(self.h, int(seq0), int(n), _lib.vp(int(ptr)), 1))
            return
        d = np.ascontiguousarray(dt, dtype=np.float64).reshape(-1)
        self._ck(self.L.sl2_set_delta_t(self.h, int(seq0), int(d.size), d.ctypes.data_as(_lib.vp), 0))

    def get_delta_t(self, seq0=0, nseq=None):
        """(dt, owed, last_used), float64 [nseq] each: the nominal time step, the time owed by skipped predicts and the step the
        last predict used (sl2_get_delta_t; synchronises)."""
        nseq = self.batch - seq0 if nseq is None else nseq
        dt, owed, used = np.zeros(nseq), np.zeros(nseq), np.zeros(nseq)
        self._ck(self.L.sl2_get_delta_t(self.h, int(seq0), int(nseq), _lib.dp(dt), _lib.dp(owed), _lib.dp(used)))
        return dt, owed, used

    def set_pause_catch_up(self, enabled=True):
        """With catch-up on, a resumed sequence predicts over its nominal step plus one for every predict it sat out; off (the
        default) clears what is owed (sl2_set_pause_catch_up)."""
        self._ck(self.L.sl2_set_pause_catch_up(self.h, int(bool(enabled))))

    def set_cameras(self, cams, seq0=0):
        """The calibration of sequences seq0, seq0 + 1, ... for every step issued from now on (sl2_set_cameras).  cams: a list of
        camera dicts (or one dict) with the engine's width / height; fku, fkv, u0, v0, kd1 finite, fku and fkv not 0, sd >= 0 -
        otherwise SL2_ERR_INVALID and nothing changes.  Consumed before the call returns; never synchronises, drops no captured
        step, does not consult the mask."""
        if isinstance(cams, dict):
            cams = [cams]
        arr = (_lib.sl2_camera * len(cams))(*[_lib.make_camera(c) for c in cams])
        self._ck(self.L.sl2_set_cameras(self.h, int(seq0), len(cams), C.cast(arr, _lib.vp)))

    def get_cameras(self, seq0=0, nseq=None):
        """A list of camera dicts, one per sequence: the calibration as the setters called so far leave it (sl2_get_cameras; the
        engine's host-side copy, no synchronisation)."""
        nseq = self.batch - seq0 if nseq is None else nseq
        arr = (_lib.sl2_camera * max(int(nseq), 1))()
        self._ck(self.L.sl2_get_cameras(self.h, int(seq0), int(nseq), C.cast(arr, _lib.vp)))
        return [dict(width=c.width, height=c.height, fku=c.fku, fkv=c.fkv, u0=c.u0, v0=c.v0, kd1=c.kd1, sd=c.sd) for c in arr[:nseq]]

    def set_groups(self, groups):
        self._ck(self.L.sl2_set_groups(self.h, int(groups)))

    @property
    def stream(self):
        """The hipStream_t (as an integer) the engine's steps are queued on: what Ingest.next wants."""
        return self.L.sl2_get_stream(self.h)

    def set_step_fusion(self, enabled=True):
        """Small maps step in three launches (default) / always one stage per launch (sl2_set_step_fusion)."""
        self._ck(self.L.sl2_set_step_fusion(self.h, int(enabled)))

    def set_graph_mode(self, enabled=True):
        self._ck(self.L.sl2_set_graph_mode(self.h, int(bool(enabled))))

    def set_search_variant(self, variant):
        self._ck(self.L.sl2_set_search_variant(self.h, int(variant)))

    def set_search_split(self, min_bands):
        """Windows of at least `min_bands` 32 x 16 bands are shared out over the wavefronts of the search launch (0 = never)."""
        self._ck(self.L.sl2_set_search_split(self.h, int(min_bands)))

    def set_update_variant(self, chol_variant=1, fwd_variant=1):
        self._ck(self.L.sl2_set_update_variant(self.h, int(chol_variant), int(fwd_variant)))

    def kalman_filter_predict(self):
        self._ck(self.L.sl2_kalman_filter_predict(self.h))

    def auto_select_n_features(self, n):
        self._ck(self.L.sl2_auto_select_n_features(self.h, int(n)))

    def make_measurements(self, frames, on_device=False, seq_stride=0):
        ptr, stride, dev, keep = self._frames_arg(frames, seq_stride, on_device)
        self._ck(self.L.sl2_make_measurements(self.h, ptr, stride, dev))
        if keep is not None:
            self.synchronize()

    def kalman_filter_update(self):
        self._ck(self.L.sl2_kalman_filter_update(self.h))

    def finish_step(self, save_trajectory=False):
        self._ck(self.L.sl2_finish_step(self.h, int(save_trajectory)))

    def synchronize(self):
        self._ck(self.L.sl2_synchronize(self.h))

    # ---- state access ------------------------------------------------------
    def total_state_sizes(self, seq0=0, nseq=None):
        nseq = self.batch - seq0 if nseq is None else nseq
        out = np.zeros(nseq, dtype=np.int32)
        self._ck(self.L.sl2_get_total_state_sizes(self.h, seq0, nseq, _lib.ip(out)))
        return out

    def total_state(self, seq):
        n = int(self.total_state_sizes(seq, 1)[0])
        x = np.zeros(n)
        self._ck(self.L.sl2_get_total_state(self.h, seq, _lib.dp(x), n))
        return x

    def total_covariance(self, seq):
        n = int(self.total_state_sizes(seq, 1)[0])
        P = np.zeros((n, n))
        self._ck(self.L.sl2_get_total_covariance(self.h, seq, _lib.dp(P), n))
        return P

    def snapshot(self, seq, traj_cursor=0, patch_from_label=0):
        """sl2_snapshot: everything the reference exposes as public members of one sequence, in ONE call (one kernel, one
        synchronisation).  Returns a dict of numpy arrays / python values decoded from the blob."""
        blob, nbytes = _lib.vp(), C.c_size_t(0)
        self._ck(self.L.sl2_snapshot(self.h, int(seq), int(traj_cursor), int(patch_from_label), C.byref(blob), C.byref(nbytes)))
        raw = C.string_at(blob.value, nbytes.value)      # the engine's pinned buffer is reused by the next call: copy out
        out = decode_snapshot(raw)
        assert out["header"].bytes == nbytes.value
        return out

    def snapshot_batch(self, seq0=0, nseq=None, sections=_lib.SL2_SNAP_ALL, cursors=None):
        """sl2_snapshot_batch, host form: the blobs of sequences seq0 .. seq0 + nseq - 1 in one call (three launches, one wait,
        one copy of exactly the packed bytes).  sections: SL2_SNAP_* bits (header, xv and Pxx always come); cursors: None or
        [nseq][2] = (traj_cursor, patch_from_label) per sequence.  Returns (snaps, offsets): a list of the dicts Engine.snapshot
        returns - an omitted section decodes as empty and the Pxy / Pyy of a feature as None without SL2_SNAP_COV - and the
        uint64 [nseq + 1] offsets of the blobs in the packed buffer."""
        raw, offsets = self.snapshot_batch_raw(seq0, nseq, sections, cursors)
        return [decode_snapshot(raw[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(offsets) - 1)], offsets

    def snapshot_bound(self, sections=_lib.SL2_SNAP_ALL):
        """sl2_snapshot_bound for this engine's shape: no blob restricted to `sections` is larger (the partial slots and the
        particle capacity as sl2_create derives them from the parameters)."""
        kpart = max(1, min(4, self._prm.max_features_to_init_at_once))
        pcap = (max(1, min(1024, self._prm.number_of_particles)) + 63) // 64 * 64
        return self.L.sl2_snapshot_bound(self.max_features, kpart, pcap, int(sections))

    def snapshot_batch_raw(self, seq0=0, nseq=None, sections=_lib.SL2_SNAP_ALL, cursors=None):
        """The packed bytes of Engine.snapshot_batch undecoded: (bytes, offsets)."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        cur = None if cursors is None else np.ascontiguousarray(cursors, dtype=np.int32).reshape(nseq, 2)
        buf = np.empty(max(self.snapshot_bound(sections), 16) * max(nseq, 1), dtype=np.uint8)
        offsets = np.zeros(max(nseq, 0) + 1, dtype=np.uint64)
        rc = self.L.sl2_snapshot_batch(self.h, int(seq0), nseq, int(sections), None if cur is None else cur.ctypes.data_as(_lib.vp),
                                       buf.ctypes.data_as(_lib.vp), buf.nbytes, offsets.ctypes.data_as(_lib.vp), 0)
        if rc == _lib.SL2_ERR_CAPACITY:      # (the shape the bound was taken for is not the engine's: ask again with the size it names)
            buf = np.empty(int(offsets[nseq]), dtype=np.uint8)
            rc = self.L.sl2_snapshot_batch(self.h, int(seq0), nseq, int(sections), None if cur is None else cur.ctypes.data_as(_lib.vp),
                                           buf.ctypes.data_as(_lib.vp), buf.nbytes, offsets.ctypes.data_as(_lib.vp), 0)
        self._ck(rc)
        return buf[:int(offsets[nseq])].tobytes(), offsets

    def snapshot_batch_device(self, out_ptr, out_bytes, offsets_ptr, seq0=0, nseq=None, sections=_lib.SL2_SNAP_ALL, cursors_ptr=None):
        """sl2_snapshot_batch, device form, for callers that hold device memory: out_ptr (16-byte aligned, out_bytes long),
        offsets_ptr (uint64 [nseq + 1]) and cursors_ptr (int32 [nseq][2] or None) are device pointers as integers.  Three launches
        on the engine's stream and no wait: a consumer on that stream (Engine.stream) needs no other ordering; if the blobs need
        more than out_bytes none is written and offsets[nseq] says how much.  Returns (out_ptr, offsets_ptr)."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        self._ck(self.L.sl2_snapshot_batch(self.h, int(seq0), nseq, int(sections), _lib.vp(int(cursors_ptr)) if cursors_ptr else None,
                                           _lib.vp(int(out_ptr)), int(out_bytes), _lib.vp(int(offsets_ptr)), 1))
        return out_ptr, offsets_ptr

    # ---- annotated frames (include/scenelib2_amd.h, "annotated frames") ----
    def overlay_item_bound(self):
        """sl2_overlay_item_bound for this engine's shape: no sequence's draw list is longer."""
        kpart = max(1, min(4, self._prm.max_features_to_init_at_once))
        return int(self.L.sl2_overlay_item_bound(self.max_features, kpart))

    def _marked_arg(self, marked, nseq):
        if marked is None:
            return None, None
        m = np.ascontiguousarray(marked, dtype=np.int32).reshape(nseq)
        return m.ctypes.data_as(_lib.vp), m

    def overlay_items(self, seq0=0, nseq=None, layers=_lib.SL2_OVERLAY_ALL, marked=None):
        """sl2_overlay_items, host form: the draw lists of sequences seq0 .. seq0 + nseq - 1 as a list of arrays of
        _lib.OVERLAY_ITEM_DTYPE.  layers: SL2_OVERLAY_* bits; marked: None or [nseq] labels (-1: none)."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        stride = self.overlay_item_bound()
        items = np.zeros((max(nseq, 1), stride), _lib.OVERLAY_ITEM_DTYPE)
        counts = np.zeros(max(nseq, 1), np.int32)
        mp, keep = self._marked_arg(marked, nseq)
        self._ck(self.L.sl2_overlay_items(self.h, int(seq0), nseq, int(layers), mp, items.ctypes.data_as(_lib.vp), stride,
                                          counts.ctypes.data_as(_lib.vp), 0))
        return [items[i, :counts[i]].copy() for i in range(nseq)]

    def draw_overlays(self, frames, seq0=0, nseq=None, layers=_lib.SL2_OVERLAY_ALL, marked=None, on_device=False, seq_stride=0,
                      out_stride=0):
        """sl2_draw_overlays with the images returned to the host: uint8 [nseq][height][width][3] (with out_stride above
        3 width height: [nseq][out_stride] bytes, the images at the start of each).  frames: uint8 [nseq][height][width] in host
        memory, or with on_device=True a device pointer (seq_stride bytes apart)."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        w, h = int(self.cam["width"]), int(self.cam["height"])
        if on_device:
            fp, stride, keep = _lib.vp(int(frames)), int(seq_stride if seq_stride else self.frame_bytes), None
        else:
            keep = np.ascontiguousarray(frames, dtype=np.uint8).reshape(nseq, -1)
            fp, stride = keep.ctypes.data_as(_lib.vp), keep.shape[1]
        ostride = int(out_stride) if out_stride else 3 * w * h
        out = np.zeros((max(nseq, 1), ostride), np.uint8)
        mp, keep_m = self._marked_arg(marked, nseq)
        self._ck(self.L.sl2_draw_overlays(self.h, int(seq0), nseq, fp, stride, int(bool(on_device)), int(layers), mp,
                                          out.ctypes.data_as(_lib.vp), ostride, 0))
        return out[:nseq].reshape(nseq, h, w, 3) if ostride == 3 * w * h else out[:nseq]

    def draw_overlays_device(self, frames_ptr, out_ptr, seq0=0, nseq=None, layers=_lib.SL2_OVERLAY_ALL, marked_ptr=None, seq_stride=0,
                             out_stride=0):
        """sl2_draw_overlays, device form: frames_ptr, out_ptr and marked_ptr (int32 [nseq] or None) are device pointers as
        integers.  Two launches on the engine's stream and no wait."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        w, h = int(self.cam["width"]), int(self.cam["height"])
        self._ck(self.L.sl2_draw_overlays(self.h, int(seq0), nseq, _lib.vp(int(frames_ptr)), int(seq_stride if seq_stride else self.frame_bytes), 1,
                                          int(layers), _lib.vp(int(marked_ptr)) if marked_ptr else None, _lib.vp(int(out_ptr)),
                                          int(out_stride if out_stride else 3 * w * h), 1))
        return out_ptr

    # ---- the rectified view (include/scenelib2_amd.h, "the rectified view") ----
    def rectify_frames(self, frames, seq0=0, nseq=None, on_device=False, seq_stride=0, out_stride=0):
        """sl2_rectify_frames with the images returned to the host: uint8 [nseq][height][width] (with out_stride above
        width height: [nseq][out_stride] bytes, the images at the start of each), sequence seq0 + i undistorted with its own
        camera (set_cameras).  frames: uint8 [nseq][height][width] in host memory, or with on_device=True a device pointer
        (seq_stride bytes apart)."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        w, h = int(self.cam["width"]), int(self.cam["height"])
        if on_device:
            fp, stride, keep = _lib.vp(int(frames)), int(seq_stride if seq_stride else self.frame_bytes), None
        else:
            keep = np.ascontiguousarray(frames, dtype=np.uint8).reshape(nseq, -1)
            fp, stride = keep.ctypes.data_as(_lib.vp), keep.shape[1]
        ostride = int(out_stride) if out_stride else w * h
        out = np.zeros((max(nseq, 1), ostride), np.uint8)
        self._ck(self.L.sl2_rectify_frames(self.h, int(seq0), nseq, fp, stride, int(bool(on_device)), out.ctypes.data_as(_lib.vp), ostride, 0))
        return out[:nseq].reshape(nseq, h, w) if ostride == w * h else out[:nseq]

    def rectify_frames_device(self, frames_ptr, out_ptr, seq0=0, nseq=None, seq_stride=0, out_stride=0):
        """sl2_rectify_frames, device form: frames_ptr and out_ptr are device pointers as integers (out must not overlap frames).
        One launch on the engine's stream and no wait."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        w, h = int(self.cam["width"]), int(self.cam["height"])
        self._ck(self.L.sl2_rectify_frames(self.h, int(seq0), nseq, _lib.vp(int(frames_ptr)), int(seq_stride if seq_stride else self.frame_bytes), 1,
                                           _lib.vp(int(out_ptr)), int(out_stride if out_stride else w * h), 1))
        return out_ptr

    def scene_item_bound(self):
        """sl2_scene_item_bound for this engine's shape: no sequence's scene list is longer."""
        kpart = max(1, min(4, self._prm.max_features_to_init_at_once))
        return int(self.L.sl2_scene_item_bound(self.max_features, kpart))

    def scene_items(self, seq0=0, nseq=None, layers=_lib.SL2_SCENE_ALL, marked=None):
        """sl2_scene_items, host form: the 3-D scene of sequences seq0 .. seq0 + nseq - 1 in their rectified images (trajectory,
        feature markers, 3-sigma ellipsoid outlines, rays of partial features) as a list of arrays of _lib.OVERLAY_ITEM_DTYPE.
        layers: SL2_SCENE_* bits; marked: None or [nseq] labels (-1: none)."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        stride = self.scene_item_bound()
        items = np.zeros((max(nseq, 1), stride), _lib.OVERLAY_ITEM_DTYPE)
        counts = np.zeros(max(nseq, 1), np.int32)
        mp, keep = self._marked_arg(marked, nseq)
        self._ck(self.L.sl2_scene_items(self.h, int(seq0), nseq, int(layers), mp, items.ctypes.data_as(_lib.vp), stride,
                                        counts.ctypes.data_as(_lib.vp), 0))
        return [items[i, :counts[i]].copy() for i in range(nseq)]

    def draw_rectified(self, frames, seq0=0, nseq=None, layers=_lib.SL2_SCENE_ALL, marked=None, on_device=False, seq_stride=0,
                       out_stride=0):
        """sl2_draw_rectified with the images returned to the host: the undistorted frames with the scene drawn over them,
        uint8 [nseq][height][width][3] (with out_stride above 3 width height: [nseq][out_stride] bytes).  frames as for
        draw_overlays."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        w, h = int(self.cam["width"]), int(self.cam["height"])
        if on_device:
            fp, stride, keep = _lib.vp(int(frames)), int(seq_stride if seq_stride else self.frame_bytes), None
        else:
            keep = np.ascontiguousarray(frames, dtype=np.uint8).reshape(nseq, -1)
            fp, stride = keep.ctypes.data_as(_lib.vp), keep.shape[1]
        ostride = int(out_stride) if out_stride else 3 * w * h
        out = np.zeros((max(nseq, 1), ostride), np.uint8)
        mp, keep_m = self._marked_arg(marked, nseq)
        self._ck(self.L.sl2_draw_rectified(self.h, int(seq0), nseq, fp, stride, int(bool(on_device)), int(layers), mp,
                                           out.ctypes.data_as(_lib.vp), ostride, 0))
        return out[:nseq].reshape(nseq, h, w, 3) if ostride == 3 * w * h else out[:nseq]

    def draw_rectified_device(self, frames_ptr, out_ptr, seq0=0, nseq=None, layers=_lib.SL2_SCENE_ALL, marked_ptr=None, seq_stride=0,
                              out_stride=0):
        """sl2_draw_rectified, device form: frames_ptr, out_ptr and marked_ptr (int32 [nseq] or None) are device pointers as
        integers.  Three launches on the engine's stream and no wait."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        w, h = int(self.cam["width"]), int(self.cam["height"])
        self._ck(self.L.sl2_draw_rectified(self.h, int(seq0), nseq, _lib.vp(int(frames_ptr)), int(seq_stride if seq_stride else self.frame_bytes), 1,
                                           int(layers), _lib.vp(int(marked_ptr)) if marked_ptr else None, _lib.vp(int(out_ptr)),
                                           int(out_stride if out_stride else 3 * w * h), 1))
        return out_ptr

    # ---- the world view (include/scenelib2_amd.h, "the world view and picking") ----
    def world_item_bound(self):
        """sl2_world_item_bound for this engine's shape: no sequence's world list is longer."""
        kpart = max(1, min(4, self._prm.max_features_to_init_at_once))
        return int(self.L.sl2_world_item_bound(self.max_features, kpart))

    @staticmethod
    def _views_arg(views, nseq):
        """One view (world_view.look_at / world_view.view) or a sequence of nseq of them, as a contiguous VIEW_DTYPE array."""
        v = np.atleast_1d(np.ascontiguousarray(views, dtype=_lib.VIEW_DTYPE)).reshape(-1)
        if v.size not in (1, nseq):
            raise ValueError("one view, or one per sequence")
        return v

    def world_items(self, views, seq0=0, nseq=None, layers=_lib.SL2_WORLD_ALL, marked=None):
        """sl2_world_items, host form: the 3-D scene of sequences seq0 .. seq0 + nseq - 1 seen through `views` (one, or one per
        sequence) - camera glyph, trajectory, feature markers, 3-sigma ellipsoid outlines, rays, axes - as (lists, extents):
        a list of arrays of _lib.OVERLAY_ITEM_DTYPE and float64 [nseq][6] = xmin, xmax, ymin, ymax, zmin, zmax of each map.
        layers: SL2_WORLD_* bits; marked: None or [nseq] labels (-1: none)."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        stride = self.world_item_bound()
        v = self._views_arg(views, nseq)
        items = np.zeros((max(nseq, 1), stride), _lib.OVERLAY_ITEM_DTYPE)
        counts = np.zeros(max(nseq, 1), np.int32)
        extents = np.zeros((max(nseq, 1), 6), np.float64)
        mp, keep = self._marked_arg(marked, nseq)
        self._ck(self.L.sl2_world_items(self.h, int(seq0), nseq, v.ctypes.data_as(_lib.vp), v.size, int(layers), mp,
                                        items.ctypes.data_as(_lib.vp), stride, counts.ctypes.data_as(_lib.vp),
                                        extents.ctypes.data_as(_lib.vp), 0))
        return [items[i, :counts[i]].copy() for i in range(nseq)], extents[:nseq]

    def draw_world(self, views, width, height, seq0=0, nseq=None, background=0, layers=_lib.SL2_WORLD_ALL, marked=None, out_stride=0):
        """sl2_draw_world with the images returned to the host: the world view of every sequence of the range over a constant
        grey background, uint8 [nseq][height][width][3] (with out_stride above 3 width height: [nseq][out_stride] bytes).  The
        size is the caller's, not the engine's."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        w, h = int(width), int(height)
        v = self._views_arg(views, nseq)
        ostride = int(out_stride) if out_stride else 3 * w * h
        out = np.zeros((max(nseq, 1), max(ostride, 1)), np.uint8)
        mp, keep_m = self._marked_arg(marked, nseq)
        self._ck(self.L.sl2_draw_world(self.h, int(seq0), nseq, v.ctypes.data_as(_lib.vp), v.size, w, h, int(background), int(layers), mp,
                                       out.ctypes.data_as(_lib.vp), ostride, 0))
        return out[:nseq].reshape(nseq, h, w, 3) if ostride == 3 * w * h else out[:nseq]

    def draw_world_device(self, views_ptr, nviews, width, height, out_ptr, seq0=0, nseq=None, background=0, layers=_lib.SL2_WORLD_ALL,
                          marked_ptr=None, out_stride=0):
        """sl2_draw_world, device form: views_ptr (nviews sl2_view records), out_ptr and marked_ptr (int32 [nseq] or None) are
        device pointers as integers.  A fill and two launches on the engine's stream and no wait."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        self._ck(self.L.sl2_draw_world(self.h, int(seq0), nseq, _lib.vp(int(views_ptr)), int(nviews), int(width), int(height), int(background),
                                       int(layers), _lib.vp(int(marked_ptr)) if marked_ptr else None, _lib.vp(int(out_ptr)),
                                       int(out_stride if out_stride else 3 * int(width) * int(height)), 1))
        return out_ptr

    def features(self, seq, include_deleted=False):
        arr = (_lib.sl2_feature_info * self.max_features)()
        cnt = C.c_int(0)
        self._ck(self.L.sl2_get_features(self.h, seq, arr, self.max_features, int(include_deleted), C.byref(cnt)))
        out = []
        for i in range(cnt.value):
            f = arr[i]
            out.append(dict(label=f.label, active=bool(f.active), selected=bool(f.selected_flag),
                            success=bool(f.successful_measurement_flag),
                            attempted=f.attempted_measurements_of_feature,
                            successful=f.successful_measurements_of_feature,
                            pos=f.position_in_total_state_vector, visible=bool(f.visible),
                            y=np.array(f.y[:]), h=np.array(f.h[:]), z=np.array(f.z[:]), nu=np.array(f.nu[:]),
                            R=float(f.R), S=np.array(f.S[:]).reshape(2, 2),
                            dh_by_dxp=np.array(f.dh_by_dxp[:]).reshape(2, 7),
                            dh_by_dy=np.array(f.dh_by_dy[:]).reshape(2, 3), xp_org=np.array(f.xp_org[:]),
                            fully_initialised=bool(f.fully_initialised_flag), state_size=int(f.state_size),
                            y_direction=np.array(f.y_direction[:])))
        return out

    def partial_feature(self, seq, index=0, capacity=1024):
        """Entry `index` of feature_init_info_vector_ of a sequence (FeatureInitInfo + particles), or None; plus the mapping
        counters of the sequence under key 'info' either way (info['n_partial'] = the vector's size)."""
        ints = np.zeros(16, dtype=np.int32)
        dbl = np.zeros(9)
        parts = np.zeros((capacity, 12))
        self._ck(self.L.sl2_get_partial_feature(self.h, seq, int(index), _lib.ip(ints), _lib.dp(dbl), _lib.dp(parts), capacity))
        info = dict(n_partial=int(ints[0]), initialised=int(ints[12]), converted=int(ints[13]), deleted=int(ints[14]),
                    uu=int(ints[5]), vv=int(ints[6]), region_defined=int(ints[7]), ustart=int(ints[8]), vstart=int(ints[9]),
                    ufinish=int(ints[10]), vfinish=int(ints[11]), created=int(ints[15]), evbest=float(dbl[8]))
        if index >= ints[0]:
            return dict(info=info, pf=None)
        n = int(ints[3])
        return dict(info=info, pf=dict(label=int(ints[1]), n_particles=n, attempts=int(ints[2]), making=bool(ints[4]),
                                       mean=float(dbl[0]), covariance=float(dbl[1]), y=dbl[2:8].copy(),
                                       particles=parts[:n].copy()))

    def partial_features(self, seq, capacity=1024):
        """All entries of feature_init_info_vector_, in the vector's order."""
        first = self.partial_feature(seq, 0, capacity)
        out = [first["pf"]] if first["pf"] is not None else []
        for k in range(1, first["info"]["n_partial"]):
            out.append(self.partial_feature(seq, k, capacity)["pf"])
        return out

    def selection(self, seq):
        labels = np.zeros(self.max_features, dtype=np.int32)
        counters = np.zeros(3, dtype=np.int32)
        self._ck(self.L.sl2_get_selection(self.h, seq, _lib.ip(labels), self.max_features, _lib.ip(counters)))
        return labels[:counters[1]].copy(), dict(visible=int(counters[0]), selected=int(counters[1]),
                                                 measurement_size=int(counters[2]))

    def trajectory(self, seq, capacity=1000):
        out = np.zeros((capacity, 3))
        cnt = C.c_int(0)
        self._ck(self.L.sl2_get_trajectory(self.h, seq, _lib.dp(out), capacity, C.byref(cnt)))
        return out[:cnt.value].copy()

    def position_log(self, seq0=0, nseq=None, capacity=1000):
        """xv[0:3] after each of the last steps: [nseq][count][3]."""
        nseq = self.batch - seq0 if nseq is None else nseq
        out = np.zeros((nseq, capacity, 3))
        cnt = C.c_int(0)
        self._ck(self.L.sl2_get_position_log(self.h, seq0, nseq, _lib.dp(out), capacity, C.byref(cnt)))
        return out.reshape(-1)[: nseq * cnt.value * 3].reshape(nseq, cnt.value, 3).copy()

    def set_feature_counters(self, seq, label, attempted, successful):
        # test hook: lives in the TEST build of the library only (include/scenelib2_amd_testing.h)
        T = _lib.load_testing()
        _lib.check(T.sl2_set_feature_counters(self.h, seq, label, attempted, successful), T)

    def debug_set_position_error(self, seq, label, err):
        # test hook (TEST build only): Q28's error of the recorded position_in_total_state_vector_, written directly
        T = _lib.load_testing()
        _lib.check(T.sl2_debug_set_position_error(self.h, seq, label, err), T)

    UPDATE_PLAN_FIELDS = ("build", "build_threads", "build_nsplit", "build_lds_bytes", "chol", "chol_panel_blocks",
                          "fwd", "fwd_nb", "fwd_group_rows")
    BUILD_FORMS = ("two-pass", "<1,4>", "<2,2>", "ahead<4>", "ahead<2>")       # sl2_update_plan.hpp: BuildForm, CholForm, FwdForm
    CHOL_FORMS = ("none", "left", "panels", "per-block")
    FWD_FORMS = ("none", "ksplit", "lds", "grouped", "re-read")

    def debug_update_plan(self, group=0):
        # test hook (TEST build only): the plan launch_update would make now for a sequence group, forms by name
        T = _lib.load_testing()
        out = np.zeros(len(self.UPDATE_PLAN_FIELDS), dtype=np.int32)
        _lib.check(T.sl2_debug_update_plan(self.h, group, _lib.ip(out), out.size), T)
        p = dict(zip(self.UPDATE_PLAN_FIELDS, (int(v) for v in out)))
        p.update(build=self.BUILD_FORMS[p["build"]], chol=self.CHOL_FORMS[p["chol"]], fwd=self.FWD_FORMS[p["fwd"]])
        return p

    def debug_raw_covariance(self, seq):
        # test hook (TEST build only): the sequence's P as the kernels hold it, [ld][ld] with padding and never-used slots
        T = _lib.load_testing()
        ld = np.zeros(1, dtype=np.int32)
        P = np.zeros((1, 1))
        if T.sl2_debug_raw_covariance(self.h, seq, _lib.dp(P), 1, _lib.ip(ld)) != _lib.SL2_ERR_CAPACITY:
            raise RuntimeError("sl2_debug_raw_covariance: no size reported")
        P = np.zeros((int(ld[0]), int(ld[0])))
        _lib.check(T.sl2_debug_raw_covariance(self.h, seq, _lib.dp(P), P.shape[0], _lib.ip(ld)), T)
        return P

    def delete_features(self, labels, seq0=0):
        """mark_feature_by_lab + delete_feature, one label per sequence (-1: none); returns the per-sequence bool."""
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        done = np.zeros(lab.size, dtype=np.int32)
        self._ck(self.L.sl2_delete_features(self.h, int(seq0), lab.size, _lib.ip(lab), _lib.ip(done)))
        return done.astype(bool)

    def initialise_feature(self, frames, uv, on_device=False, seq_stride=0):
        """MonoSLAM::InitialiseFeature at (uu_, vv_) = uv[s] for every sequence (u < 0: skip); returns created [batch]."""
        ptr, stride, dev, keep = self._frames_arg(frames, seq_stride, on_device)
        sel = np.ascontiguousarray(uv, dtype=np.int32).reshape(self.batch, 2)
        created = np.zeros(self.batch, dtype=np.int32)
        self._ck(self.L.sl2_initialise_feature(self.h, ptr, stride, dev, _lib.ip(sel), _lib.ip(created)))
        return created.astype(bool)

    def initialise_auto_feature(self, frames, on_device=False, seq_stride=0):
        """MonoSLAM::InitialiseAutoFeature for every sequence; returns created [batch]."""
        ptr, stride, dev, keep = self._frames_arg(frames, seq_stride, on_device)
        created = np.zeros(self.batch, dtype=np.int32)
        self._ck(self.L.sl2_initialise_auto_feature(self.h, ptr, stride, dev, _lib.ip(created)))
        return created.astype(bool)

    def save_patch(self, seq, label, path):
        """MonoSLAM::SavePatch: Feature::patch_ of the feature with this label as PNG (or PGM by extension)."""
        self._ck(self.L.sl2_save_patch(self.h, int(seq), int(label), os.fsencode(path)))

    def feature_patch(self, seq, label):
        """Feature::patch_ of the feature with this label (11x11 uint8)."""
        out = np.zeros((11, 11), dtype=np.uint8)
        self._ck(self.L.sl2_get_feature_patch(self.h, int(seq), int(label), _lib.u8p(out)))
        return out

    def status_flags(self):
        out = np.zeros(self.batch, dtype=np.int32)
        self._ck(self.L.sl2_get_status_flags(self.h, 0, self.batch, _lib.ip(out)))
        return out

    def step_stats(self, seq0=0, nseq=None):
        """The filter-consistency record of the last completed update for sequences [seq0, seq0 + nseq) in ONE launch and one
        synchronisation (sl2_get_step_stats): a NumPy structured array (_lib.STEP_STATS_DTYPE) with fields stepped,
        status_flags, sequence_steps, n_features, n_partial, n_visible, n_selected, n_matched, dof, worst_label, nis, log_det_S,
        min_pivot, max_pivot, worst_feature_d2, position_var.  nis is chi-square with dof degrees of freedom for a consistent
        filter; the bounds are the caller's (scipy.stats.chi2.ppf, or a table)."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        out = np.zeros(max(nseq, 1), dtype=_lib.STEP_STATS_DTYPE)
        self._ck(self.L.sl2_get_step_stats(self.h, int(seq0), nseq, out.ctypes.data_as(_lib.vp), 0))
        return out[:nseq]

    def step_stats_device(self, dev_ptr, seq0=0, nseq=None):
        """The same records into device memory (96 bytes each, 8-byte aligned): the launch only, on the engine's stream, no
        synchronisation - for a policy kernel of the caller's, or set_active(on_device=True)."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        self._ck(self.L.sl2_get_step_stats(self.h, int(seq0), nseq, _lib.vp(int(dev_ptr)), 1))

    # ---- save / restore / copy / reset of sequences (sl2_save_sequences ...) -------
    def sequence_blob_capacity(self):
        """Upper bound in bytes of one sequence blob of this engine (a multiple of 64)."""
        return int(self.L.sl2_sequence_blob_capacity(self.h))

    def save_sequences(self, seq0=0, nseq=None):
        """The complete state of sequences [seq0, seq0 + nseq) as one `bytes` blob each (self-describing: see
        sl2_sequence_blob_header).  The engine is not changed."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        cap = self.sequence_blob_capacity()
        buf = np.zeros((max(nseq, 1), cap), dtype=np.uint8)
        sizes = np.zeros(max(nseq, 1), dtype=np.uint64)
        self._ck(self.L.sl2_save_sequences(self.h, int(seq0), nseq, buf.ctypes.data_as(_lib.vp), cap, 0,
                                           sizes.ctypes.data_as(C.POINTER(C.c_uint64))))
        return [buf[i, :int(sizes[i])].tobytes() for i in range(nseq)]

    def load_sequences(self, blobs, seq0=0):
        """Blobs of save_sequences (of this or any engine they fit) into sequences seq0, seq0 + 1, ...  Every header is checked
        before anything is written: a blob that is malformed or does not fit raises Sl2Error and leaves the engine untouched."""
        blobs = [blobs] if isinstance(blobs, (bytes, bytearray, memoryview)) else list(blobs)
        stride = max(256, max((len(b) for b in blobs), default=0))
        stride = (stride + 63) // 64 * 64
        buf = np.zeros((max(len(blobs), 1), stride), dtype=np.uint8)
        for i, b in enumerate(blobs):
            a = np.frombuffer(bytes(b), dtype=np.uint8)
            if a.size >= 256 and _lib.sl2_sequence_blob_header.from_buffer_copy(a[:256].tobytes()).bytes > a.size:
                raise _lib.Sl2Error(_lib.SL2_ERR_INVALID, "sequence blob %d: bytes: the blob is truncated (%d bytes given)" % (i, a.size))
            buf[i, :a.size] = a
        self._ck(self.L.sl2_load_sequences(self.h, int(seq0), len(blobs), buf.ctypes.data_as(_lib.vp), stride, 0))

    def save_sequences_device(self, dev_ptr, blob_stride, seq0=0, nseq=None):
        """Blobs into device memory (dev_ptr: 64-byte aligned, blob_stride >= sequence_blob_capacity()): one launch on the
        engine's stream, asynchronous."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        self._ck(self.L.sl2_save_sequences(self.h, int(seq0), nseq, _lib.vp(int(dev_ptr)), int(blob_stride), 1, None))

    def load_sequences_device(self, dev_ptr, blob_stride, seq0=0, nseq=None):
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        self._ck(self.L.sl2_load_sequences(self.h, int(seq0), nseq, _lib.vp(int(dev_ptr)), int(blob_stride), 1))

    def copy_sequences(self, src, src_seq0, nseq, dst_seq0):
        """Sequences [src_seq0, src_seq0 + nseq) of engine `src` (may be this engine) into [dst_seq0, ...) of this one, on
        the device."""
        self._ck(self.L.sl2_copy_sequences(self.h, int(dst_seq0), src.h, int(src_seq0), int(nseq)))

    def reset_sequences(self, seq0=0, nseq=None):
        """The sequences become what a fresh engine holds; set the vehicle state and add features next."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        self._ck(self.L.sl2_reset_sequences(self.h, int(seq0), nseq))

    # ---- profiling -----------------------------------------------------------
    def set_profile_focus(self, names=""):
        self._ck(self.L.sl2_set_profile_focus(self.h, names.encode() if names else None))

    def set_profiling(self, level):
        """0 off, 1 roofline kernels only, 2 every launch."""
        self._ck(self.L.sl2_set_profiling(self.h, int(level)))

    def reset_kernel_times(self):
        self._ck(self.L.sl2_reset_kernel_times(self.h))

    def kernel_times(self):
        n = self.L.sl2_kernel_count(self.h)
        out = {}
        for i in range(n):
            name = C.c_char_p()
            ms = C.c_double(0)
            cnt = C.c_int64(0)
            self._ck(self.L.sl2_get_kernel_time(self.h, i, C.byref(name), C.byref(ms), C.byref(cnt)))
            out[name.value.decode()] = dict(total_ms=ms.value, launches=cnt.value)
        return out

    def placement(self):
        """sl2_get_placement: how sl2_create placed the large matrices (candidates probed, probe ms of the kept P, V^T, A^T, S and
        of the slowest candidate of each size); zeros for an engine too small for it to matter."""
        w = np.zeros(10)
        self._ck(self.L.sl2_get_placement(self.h, _lib.dp(w), w.size))
        keys = ["candidates_of_P", "kept_P_ms", "kept_Vt_ms", "kept_At_ms", "kept_S_ms", "slowest_P_ms", "slowest_A_ms", "slowest_S_ms",
                "k_syrk_on_kept_pair_ms", "k_syrk_on_slowest_pair_ms"]
        return dict(zip(keys, w.tolist()))

    def step_work(self):
        w = np.zeros(13)
        self._ck(self.L.sl2_get_step_work(self.h, _lib.dp(w), w.size))
        keys = ["window_bytes", "searched", "candidates", "sum_m", "sum_m2", "sum_m3", "sum_n", "sum_nm", "sum_nnm",
                "sum_nmm", "search_fallbacks", "search_tiles", "search_shared"]
        return dict(zip(keys, w.tolist()))


class Feature:
    """Read-only view with the member names of SceneLib2::Feature (feature.h:78-142)."""

    def __init__(self, d, patch=None):
        self.label_ = d["label"]
        self.y_ = d["y"]
        self.xp_org_ = d["xp_org"]
        self.h_ = d["h"]
        self.z_ = d["z"]
        self.nu_ = d["nu"]
        self.S_ = d["S"]
        self.R_ = np.eye(2) * d["R"]
        dh = np.zeros((2, 13))
        dh[:, :7] = d["dh_by_dxp"]
        self.dh_by_dxv_ = dh
        self.dh_by_dy_ = d["dh_by_dy"]
        self.selected_flag_ = d["selected"]
        self.successful_measurement_flag_ = d["success"]
        self.attempted_measurements_of_feature_ = d["attempted"]
        self.successful_measurements_of_feature_ = d["successful"]
        self.position_in_total_state_vector_ = d["pos"]
        self.fully_initialised_flag_ = d.get("fully_initialised", True)
        self.patch_ = patch


class MonoSLAM:
    """Single-sequence MonoSLAM with the reference's public surface (monoslam.h:69-219)."""

    kBoxSize_ = 11
    kNoSigma_ = 3.0
    kCorrThresh2_ = 0.40
    kCorrelationSigmaThreshold_ = 10.0

    def __init__(self, max_features=64, device=0):
        self._max_features = max_features
        self._device = device
        self._engine = None
        self._patches = {}
        self.camera_ = None
        self.uu_, self.vv_ = 0, 0                   # image selection (set by the GUI's mouse handler in the reference)
        self.location_selected_flag_ = False
        self.marked_feature_label_ = -1             # monoslam.h:171
        self._last_3d = None                        # Picker: the view, size and layers of the last Draw3dScene ...
        self._last_ar = None                        # ... and the kind and layers of the last DrawAR
        self._converter = None                      # SetFrameSource: raw camera frames in front of GoOneStep
        self._frame_dev = None
        self._frame_filter = "linear"               # SetFrameFilter
        self._frame_gate = None                     # SetFrameGate: the gate in front of every step
        self._monitor = None
        self._gate_active_dev = None
        self._host_digest = None                    # of the last HOST frame examined
        self._last_frame_verdict = 0

    # MonoSLAM::Init(config_path) — monoslam.cpp:1574-1969
    def Init(self, config_path, template_dirs=()):
        cfg = load_config(config_path)
        self.InitFromValues(cfg["cam"], cfg["params"], cfg["xv"], cfg["Pxx"])
        for f in cfg["features"]:
            self.AddNewKnownFeature(f["y"], f["xp_org"], resolve_identifier(f, template_dirs))
        return self

    def InitFromValues(self, cam, params, xv, Pxx):
        self.camera_ = dict(cam)
        self.kDeltaT_ = params["delta_t"]
        self.kNumberOfFeaturesToSelect_ = params["number_of_features_to_select"]
        self._engine = Engine(cam, params, 1, self._max_features, self._device)
        self._drop_frame_gate()                     # (sized by the camera of the last Init; the new engine has no catch-up set)
        self._engine.set_vehicle_state(np.asarray(xv).reshape(1, 13), np.asarray(Pxx).reshape(1, 13, 13))
        return self

    def SetDeltaT(self, delta_t):
        """kDeltaT_ from the next GoOneStep on (the reference fixes it at Init; a camera whose frame rate changes does not)."""
        self._engine.set_delta_t(float(delta_t))
        self.kDeltaT_ = float(delta_t)

    # Camera::SetCameraParameters(width, height, fku, fkv, u0, v0, kd1, sd) — camera.cpp:49-62
    def SetCameraParameters(self, width, height, fku, fkv, u0, v0, kd1, sd):
        """camera_'s calibration from the next GoOneStep on (a recalibrated camera, or another unit of the same model).  The image
        size is fixed at Init: width / height must be the ones it was given."""
        cam = dict(width=int(width), height=int(height), fku=float(fku), fkv=float(fkv), u0=float(u0), v0=float(v0),
                   kd1=float(kd1), sd=int(sd))
        self._engine.set_cameras([cam])
        self.camera_.update(cam)

    # MonoSLAM::AddNewKnownFeature(y, xp, identifier) — monoslam.cpp:1278-1291
    def AddNewKnownFeature(self, y, xp, identifier):
        patch = read_pgm(identifier) if isinstance(identifier, str) else np.asarray(identifier, dtype=np.uint8)
        if patch.shape != (11, 11):
            raise ValueError("template must be 11x11")
        label = len(self._patches)
        self._engine.add_known_features(np.asarray(y).reshape(1, 1, 3), np.asarray(xp).reshape(1, 1, 7),
                                        patch.reshape(1, 1, 11, 11))
        self._patches[label] = patch

    # MonoSLAM::GoOneStep(frame, save_trajectory, enable_mapping) — monoslam.cpp:108-180
    def GoOneStep(self, frame, save_trajectory=False, enable_mapping=False):
        f = np.ascontiguousarray(frame, dtype=np.uint8)
        if f.size != self._engine.frame_bytes:
            raise ValueError("frame must be %d x %d 8-bit single channel" % (self.camera_["width"], self.camera_["height"]))
        if self._frame_gate is not None:            # a host frame: the two host forms for its one frame
            from . import frame_monitor
            rec = frame_monitor.frame_stats_host(f.reshape(-1), self.camera_["width"], self.camera_["height"])
            self._last_frame_verdict = frame_monitor.frame_verdict_host(rec, self._frame_gate, self._host_digest is not None,
                                                                        self._host_digest or 0)
            self._host_digest = int(rec["digest"])
            self._engine.set_active([self._last_frame_verdict == 0])
        self._engine.go_one_step(f.reshape(1, -1), save_trajectory, enable_mapping)
        return self._after_step(enable_mapping)

    def SetFrameGate(self, gate, catch_up=False):
        """A gate in front of every step (frame_monitor.make_gate: a dict of its thresholds): from the next GoOneStep / GoOneStepRaw
        on the frame is examined first, and a frame the gate rejects - the camera repeated its buffer, delivered a black or
        saturated frame, a smeared one - is not shown to the filter: the step leaves it as it was.  GoOneStepRaw's device frame is
        examined on the engine's stream and its verdict feeds the mask on the device, with no wait in between; GoOneStep's host
        frame goes through the host forms.  The previous digest is kept per kind of frame.  catch_up: the predict that follows a
        rejected frame covers the gap (Engine.set_pause_catch_up).  Without this call nothing changes."""
        from . import frame_monitor
        if self._engine is None:
            raise RuntimeError("MonoSLAM.SetFrameGate: call Init first")
        g = frame_monitor.make_gate(gate)
        if self._monitor is None:
            self._monitor = frame_monitor.FrameMonitor(self._device, 1, self.camera_["width"], self.camera_["height"])
            self._gate_active_dev = _lib.DeviceBuffer(1, self._device)
        self._monitor.set_gates([g])
        self._engine.set_pause_catch_up(bool(catch_up))
        self._frame_gate = g

    def _drop_frame_gate(self):
        if self._monitor is not None:
            self._monitor.close()
            self._gate_active_dev.free()
        self._monitor = self._gate_active_dev = self._frame_gate = self._host_digest = None
        self._last_frame_verdict = 0

    def LastFrameVerdict(self):
        """The verdict of the last frame a step was asked to take (frame_monitor.SL2_FRAME_* bits; 0: it passed, or no gate)."""
        return self._last_frame_verdict

    def _after_step(self, enable_mapping):
        # the reference's feature_list_ is unbounded; the engine holds at most max_features LIVE features per sequence
        # (deleted ones give their slots back): a full map must not pass silently (SL2_STATUS_LABELS_EXHAUSTED)
        if enable_mapping:
            full = bool(int(self._engine.status_flags()[0]) & 2)
            rose, self._map_full = full and not getattr(self, "_map_full", False), full
            if rose:          # (once per episode: the step itself has been applied; the bit clears when a slot frees up)
                raise RuntimeError("MonoSLAM: all %d feature slots hold live features (max_features); mapping cannot "
                                   "initialise features until one is deleted - create the engine with a larger max_features"
                                   % self._max_features)
        return True  # the reference always returns true (monoslam.cpp:179)

    def SetFrameSource(self, width, height, pitch, format):
        """What the camera delivers (UsbCamGrabber, usbcamgrabber.cpp:75-113): its size, row pitch in bytes and pixel format
        (convert.SL2_PIX_* or a name of convert.FORMATS: "uyvy", "rgb24", "gray12", "bayer_rggb8" ...).  GoOneStepRaw converts such frames to the engine's grey image on the
        device.  The converter and the device frame are created on the first call."""
        self._ensure_converter()
        self._converter.set_sources([dict(width=width, height=height, pitch=pitch, format=format)])

    def _ensure_converter(self):
        from . import convert
        if self._converter is None:
            self._converter = convert.FrameConverter(self._device, 1, self.camera_["width"], self.camera_["height"])
            self._frame_dev = _lib.DeviceBuffer(self._engine.frame_bytes, self._device)
            self._converter.set_filters([self._frame_filter])

    def SetLens(self, lens, target):
        """A camera whose lens the filter's model does not describe (OpenCV's k1 k2 p1 p2 k3 [k4 k5 k6], or its fisheye k1 .. k4):
        GoOneStepRaw then reads every frame through the map from `target` into the lens's image (convert.lens_map), in place of
        the resize filter, and the filter runs with `target` (SetCameraParameters).  lens: a dict as for convert.make_lens; target:
        a camera dict of the engine's image size (convert.pinhole_camera gives the obvious one; a target with kd1 > 0 keeps more of
        a wide lens's field).  Before or after SetFrameSource, whose size must be the lens's."""
        from . import convert
        if (int(target["width"]), int(target["height"])) != (self.camera_["width"], self.camera_["height"]):
            raise ValueError("MonoSLAM.SetLens: the target's size is not the engine's image size")
        ln = convert.make_lens(lens)
        xy = convert.lens_map(ln, target)
        self._ensure_converter()
        self._converter.set_remaps([-1])                    # (a slot in use keeps its size)
        self._converter.set_map(0, ln.width, ln.height, xy)
        self._converter.set_remaps([0])
        self.SetCameraParameters(target["width"], target["height"], target["fku"], target["fkv"], target["u0"], target["v0"],
                                 target["kd1"], target["sd"])

    def SetFrameFilter(self, filter):
        """How GoOneStepRaw brings the camera's frame to the engine's size: "linear" (the reference's plain INTER_LINEAR, the
        default) or "area", the exact box average for cameras much larger than the engine's image (convert.FILTERS or
        SL2_RESIZE_*).  Before or after SetFrameSource; "area" with a source smaller than the engine's image is refused by
        whichever call comes second."""
        from . import convert
        if (filter.lower() if isinstance(filter, str) else filter) not in list(convert.FILTERS) + list(convert.FILTERS.values()):
            raise ValueError("MonoSLAM.SetFrameFilter: unknown filter %r" % (filter,))
        if self._converter is not None:
            self._converter.set_filters([filter])
        self._frame_filter = filter

    def GoOneStepRaw(self, raw, save_trajectory=False, enable_mapping=False, on_device=False):
        """sl2_convert_frames, then GoOneStep on the converted device frame.  raw: the camera's bytes as a uint8 array, or with
        on_device=True a (device pointer, bytes) pair."""
        if self._converter is None:
            raise RuntimeError("MonoSLAM.GoOneStepRaw: call SetFrameSource first")
        keep = self._converter.convert(raw if not on_device else tuple(raw), self._frame_dev, stream=self._engine.stream)
        if self._frame_gate is not None:            # examine, then the mask in device form: no wait in between
            self._monitor.examine(self._frame_dev, active_out=self._gate_active_dev, stream=self._engine.stream)
            self._engine.set_active((self._gate_active_dev.ptr, 1), on_device=True)
        self._engine.go_one_step(self._frame_dev.ptr, save_trajectory, enable_mapping, on_device=True)
        if keep is not None:
            self._engine.synchronize()  # the host buffer must outlive the copy queued in front of the step
        if self._frame_gate is not None:
            self._last_frame_verdict = int(self._monitor.read()[1][0])
        return self._after_step(enable_mapping)

    # GraphicTool::DrawRawAR(frame, chk_display_2d_descriptors, chk_display_2d_search_regions, chk_display_initialisation)
    # — graphictool.cpp:285-364, without OpenGL
    def DrawRawAR(self, frame, out_rgb=None, chk_display_2d_descriptors=True, chk_display_2d_search_regions=True,
                  chk_display_initialisation=True):
        """The frame annotated with the search ellipses, the templates, a partially initialised feature's particle ellipses and
        the initialisation boxes (sl2_draw_overlays): uint8 [height][width][3], R, G, B; also written into out_rgb if given.
        marked_feature_label_ is drawn green."""
        layers = (_lib.SL2_OVERLAY_SEARCH_REGIONS if chk_display_2d_search_regions else 0) | \
                 (_lib.SL2_OVERLAY_DESCRIPTORS if chk_display_2d_descriptors else 0) | \
                 (_lib.SL2_OVERLAY_INITIALISATION if chk_display_initialisation else 0)
        self._last_ar = ("raw", layers)             # (Picker: the check boxes of the last call)
        img = self._engine.draw_overlays(self._frame(frame), 0, 1, layers, [self.marked_feature_label_])[0]
        if out_rgb is not None:
            out_rgb[...] = img
        return img

    # GraphicTool::DrawRectifiedAR(frame, chk_display_trajectory, chk_display_3d_features, chk_display_3d_uncertainties)
    # — graphictool.cpp:222-283, without OpenGL
    def DrawRectifiedAR(self, frame, out_rgb=None, chk_display_trajectory=True, chk_display_3d_features=True,
                        chk_display_3d_uncertainties=True):
        """The frame with the lens distortion removed and, over it, the trajectory, the 3-D features, their 3-sigma ellipsoids
        and the rays of partially initialised features (sl2_draw_rectified): uint8 [height][width][3], R, G, B; also written
        into out_rgb if given.  marked_feature_label_ is drawn green."""
        layers = (_lib.SL2_SCENE_TRAJECTORY if chk_display_trajectory else 0) | \
                 (_lib.SL2_SCENE_FEATURES if chk_display_3d_features else 0) | \
                 (_lib.SL2_SCENE_UNCERTAINTIES if chk_display_3d_uncertainties else 0)
        self._last_ar = ("rectified", layers)
        img = self._engine.draw_rectified(self._frame(frame), 0, 1, layers, [self.marked_feature_label_])[0]
        if out_rgb is not None:
            out_rgb[...] = img
        return img

    # GraphicTool::DrawAR — graphictool.cpp:177-220: the rectified view or the raw one, by the example's check box
    def DrawAR(self, frame, out_rgb=None, chk_rectify_image_display=False, chk_display_trajectory=True, chk_display_3d_features=True,
               chk_display_3d_uncertainties=True, chk_display_2d_descriptors=True, chk_display_2d_search_regions=True,
               chk_display_initialisation=True):
        if chk_rectify_image_display:
            return self.DrawRectifiedAR(frame, out_rgb, chk_display_trajectory, chk_display_3d_features, chk_display_3d_uncertainties)
        return self.DrawRawAR(frame, out_rgb, chk_display_2d_descriptors, chk_display_2d_search_regions, chk_display_initialisation)

    # GraphicTool::Draw3dScene(chk_display_trajectory, chk_display_3d_features, chk_display_3d_uncertainties)
    # — graphictool.cpp:113-175, without OpenGL: the view is the caller's (world_view.look_at), not a GL model-view matrix
    def Draw3dScene(self, view, out_rgb=None, width=None, height=None, chk_display_trajectory=True, chk_display_3d_features=True,
                    chk_display_3d_uncertainties=True):
        """The map, the trajectory and the camera seen through `view` over a black background (sl2_draw_world): uint8
        [height][width][3], R, G, B (the camera's size by default); also written into out_rgb if given.  The camera is always
        drawn and the axes with the features, as in the reference; marked_feature_label_ is drawn green."""
        w = int(self.camera_["width"] if width is None else width)
        h = int(self.camera_["height"] if height is None else height)
        layers = (_lib.SL2_WORLD_TRAJECTORY if chk_display_trajectory else 0) | \
                 (_lib.SL2_WORLD_FEATURES | _lib.SL2_WORLD_AXES if chk_display_3d_features else 0) | \
                 (_lib.SL2_WORLD_UNCERTAINTIES if chk_display_3d_uncertainties else 0) | _lib.SL2_WORLD_CAMERA
        self._last_3d = (np.array(view, dtype=_lib.VIEW_DTYPE), w, h, layers)
        img = self._engine.draw_world(view, w, h, 0, 1, 0, layers, [self.marked_feature_label_])[0]
        if out_rgb is not None:
            out_rgb[...] = img
        return img

    # GraphicTool::Picker(x, y, ..., threed) — graphictool.cpp:1475-1571: the GL name (label + 1) under the click, 0 for none
    def Picker(self, x, y, threed=True):
        """The feature under pixel (x, y) of the last Draw3dScene (threed) or DrawAR image, image coordinates with y downwards:
        the list of that call is rebuilt from the current state with the remembered check boxes and view, and
        sl2_pick_items_host answers.  Returns label + 1, the reference's name convention, or 0:
        mark_feature_by_lab(Picker(x, y) - 1) reads as in pangolin_util.cpp."""
        from . import world_view
        if threed:
            if self._last_3d is None:
                return 0
            view, w, h, layers = self._last_3d
            items = self._engine.world_items(view, 0, 1, layers)[0][0]
        else:
            if self._last_ar is None:
                return 0
            kind, layers = self._last_ar
            w, h = int(self.camera_["width"]), int(self.camera_["height"])
            items = (self._engine.overlay_items(0, 1, layers) if kind == "raw" else self._engine.scene_items(0, 1, layers))[0]
        return world_view.pick_items_host(w, h, items, x, y, npatches=self._engine.max_features)[0] + 1

    def _frame(self, frame):
        f = np.ascontiguousarray(frame, dtype=np.uint8)
        if f.size != self._engine.frame_bytes:
            raise ValueError("frame must be %d x %d 8-bit single channel" % (self.camera_["width"], self.camera_["height"]))
        return f.reshape(1, -1)

    # MonoSLAM::InitialiseFeature(frame) at (uu_, vv_) — monoslam.cpp:1211-1235
    def InitialiseFeature(self, frame):
        return bool(self._engine.initialise_feature(self._frame(frame), [[self.uu_, self.vv_]])[0])

    # MonoSLAM::InitialiseAutoFeature(frame) — monoslam.cpp:1535-1541
    def InitialiseAutoFeature(self, frame):
        created = bool(self._engine.initialise_auto_feature(self._frame(frame))[0])
        info = self._engine.partial_feature(0)["info"]
        if created or info["region_defined"]:   # (a refused call - a partially initialised feature is still in flight: no region
            self.uu_, self.vv_ = info["uu"], info["vv"]          # was searched - leaves the selection alone)
            self.location_selected_flag_ = True
        return created

    # MonoSLAM::mark_feature_by_lab — monoslam.cpp:743-768
    def mark_feature_by_lab(self, lab):
        if lab == -1 or any(f.label_ == lab for f in self.feature_list_):
            self.marked_feature_label_ = lab

    # MonoSLAM::delete_feature — monoslam.cpp:770-812
    def delete_feature(self):
        if self.marked_feature_label_ == -1:
            return False
        done = bool(self._engine.delete_features([self.marked_feature_label_])[0])
        if done:
            self.marked_feature_label_ = -1
        return done

    # MonoSLAM::SavePatch — monoslam.cpp:1551-1572 (writes "patch.png" in the working directory)
    def SavePatch(self, path="patch.png"):
        if self.marked_feature_label_ == -1 or not any(f.label_ == self.marked_feature_label_ for f in self.feature_list_):
            return False
        self._engine.save_patch(0, self.marked_feature_label_, path)
        return True

    # The filter as a file: the sequence blob of sl2_save_sequences (not in the reference, which cannot stop and resume).
    def SaveState(self, path):
        with open(path, "wb") as f:
            f.write(self._engine.save_sequences(0, 1)[0])

    # Into an object that was initialised with the same camera and parameters (InitFromValues / Init); its map is replaced.
    def LoadState(self, path):
        with open(path, "rb") as f:
            self._engine.load_sequences([f.read()], 0)
        self._patches = {d["label"]: self._engine.feature_patch(0, d["label"]) for d in self._engine.features(0)}
        self._map_full = bool(int(self._engine.status_flags()[0]) & 2)

    @property
    def xv_(self):
        return self._engine.get_vehicle_state(0, 1)[0][0]

    @property
    def Pxx_(self):
        return self._engine.get_vehicle_state(0, 1)[1][0]

    @property
    def feature_list_(self):
        return [Feature(d, self._patches.get(d["label"])) for d in self._engine.features(0)]

    @property
    def selected_feature_list_(self):
        labels, _ = self._engine.selection(0)
        by_label = {f.label_: f for f in self.feature_list_}
        return [by_label[l] for l in labels if l in by_label]

    @property
    def number_of_visible_features_(self):
        return self._engine.selection(0)[1]["visible"]

    @property
    def successful_measurement_vector_size_(self):
        return self._engine.selection(0)[1]["measurement_size"]

    # Not in the reference: the health of the last KalmanFilterUpdate (sl2_get_step_stats) as a dict - nis, dof, log_det_S,
    # min_pivot, max_pivot, worst_label, worst_feature_d2, position_var and the step's counts
    @property
    def step_stats_(self):
        r = self._engine.step_stats(0, 1)[0]
        return {n: r[n].item() for n in r.dtype.names if n != "reserved"}

    @property
    def total_state_size_(self):
        return int(self._engine.total_state_sizes(0, 1)[0])

    @property
    def trajectory_store_(self):
        return self._engine.trajectory(0)

    def construct_total_state(self):
        return self._engine.total_state(0)

    def construct_total_covariance(self):
        return self._engine.total_covariance(0)

    # MonoSLAM::print_robot_state — monoslam.cpp:1543-1549
    def print_robot_state(self):
        print("[Robot state]")
        print(self.xv_)
        print("[Robot covariance]")
        print(self.Pxx_)
