"""bench.py's host-side pieces that need no GPU: the options of a plain and a --full run, the camera paths shared out over
worker processes, and what --dump-outputs writes (against a stand-in engine)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args(monkeypatch, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse_args()


def test_plain_run_is_the_default_and_impossible_step_counts_are_refused(monkeypatch):
    a = _args(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = _args(monkeypatch, ["--steps", "7", "--warmup", "2", "--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            _args(monkeypatch, bad)


def test_specs_from_worker_processes_are_the_specs(monkeypatch):
    import bench
    from scenelib2_amd import synth
    cam = synth.default_camera(320, 240)
    ids = list(range(5, 13))
    one = bench._specs_of((cam, 20, 30, ids, {}))
    monkeypatch.setattr(bench, "SPEC_SEQFRAMES_PER_WORKER", 60)     # 8 sequences x 31 poses: several workers
    many = bench.make_specs(cam, 20, 30, np.array(ids), {})
    assert len(many) == len(one)
    for s, t in zip(one, many):
        assert s.seed == t.seed
        for name in ("poses", "feat_px", "feat_y", "xv0", "Pxx0", "tex_origin"):
            assert np.array_equal(getattr(s, name), getattr(t, name)), name


def test_specs_workers_do_not_run_the_callers_main(tmp_path):
    """A script that calls into bench at top level, with no __main__ guard (scripts/me_trace.py calls bench.main() so): the
    workers must not run it again - they are fresh interpreters that import bench as a module."""
    script = tmp_path / "unguarded.py"
    script.write_text("import sys\nsys.path.insert(0, %r)\nimport numpy as np\nimport bench\nfrom scenelib2_amd import synth\n"
                      "bench.SPEC_SEQFRAMES_PER_WORKER = 60\n"
                      "specs = bench.make_specs(synth.default_camera(320, 240), 20, 30, np.arange(8), {})\n"
                      "print('ran', len(specs), flush=True)\n" % ROOT)
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["ran", "8"]                   # printed once: no worker re-ran the script


class _StandIn:
    """The getters dump_outputs reads, over fixed random states."""

    def __init__(self, batch, sizes, max_features):
        self.batch, self.max_features = batch, max_features
        self.sizes = np.asarray(sizes, dtype=np.int32)
        r = np.random.default_rng(1)
        self.x = [r.standard_normal(n) for n in self.sizes]
        self.P = [r.standard_normal((n, n)) for n in self.sizes]

    def get_vehicle_state(self):
        return np.stack([x[:13] for x in self.x]), np.stack([P[:13, :13] for P in self.P])

    def total_state_sizes(self):
        return self.sizes.copy()

    def total_state(self, b):
        return self.x[b]

    def total_covariance(self, b):
        return self.P[b]

    def features(self, b):
        return [dict(label=i, visible=True, selected=i % 2 == 0, success=i % 3 == 0, z=np.array([i, b]), h=np.array([b, i]))
                for i in range((self.sizes[b] - 13) // 3)]


def test_dump_outputs_writes_float64_within_the_budget(tmp_path):
    import bench
    eng = _StandIn(40, [13 + 3 * (k % 5) for k in range(40)], 8)
    total = bench.dump_outputs(eng, str(tmp_path / "a"))
    bench.dump_outputs(eng, str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "vehicle_state.npy" in files
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    assert total == sum(a.nbytes for a in got.values()) <= 64 << 20
    for f, a in got.items():
        assert a.dtype == np.float64, f
        assert np.array_equal(a, np.load(tmp_path / "b" / f)), f         # the sample is seeded
    assert np.array_equal(got["vehicle_state.npy"], eng.get_vehicle_state()[0])
    seqs = got["state_sequences.npy"].astype(int)
    assert seqs.size == 16 and np.all(np.diff(seqs) > 0)
    for j, b in enumerate(seqs):
        n = eng.sizes[b]
        assert got["state_size.npy"][j] == n
        assert np.array_equal(got["total_state.npy"][j, :n], eng.x[b]) and not got["total_state.npy"][j, n:].any()
        assert np.array_equal(got["total_covariance.npy"][j, :n, :n], eng.P[b])
        m = got["feature_measurements.npy"][j]
        k = (n - 13) // 3
        assert np.array_equal(m[:k, 0], np.arange(k)) and (m[k:, 0] == -1).all()
        assert np.array_equal(m[:k, 4:6], np.stack([np.arange(k), np.full(k, b)], axis=1).reshape(k, 2))


def test_dump_outputs_samples_rows_of_a_covariance_too_large_for_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)                  # 512 KiB for covariances: one 300 x 300 is 703 KiB
    eng = _StandIn(3, [300, 300, 300], 100)
    bench.dump_outputs(eng, str(tmp_path))
    P = np.load(tmp_path / "total_covariance.npy")
    rows = np.load(tmp_path / "covariance_rows.npy").astype(int)
    b = int(np.load(tmp_path / "state_sequences.npy")[0])
    assert P.shape == (1, rows.size, 300) and 0 < rows.size < 300 and P.nbytes <= (1 << 20) // 2
    assert np.array_equal(P[0], eng.P[b][rows])


class _Logging:
    """sl2_get_position_log's contract: xv[0:3] after the last min(capacity, steps done, 1000) steps, oldest first."""

    def __init__(self, nseq):
        self.nseq, self.steps = nseq, 0

    @staticmethod
    def truth(nseq, frames):                 # position after frame k (1-based) of sequence s
        k = np.arange(1, frames + 1)[None, :, None]
        return np.broadcast_to(k * 1.0 + np.arange(nseq)[:, None, None] * 1e4 + np.array([0.0, 0.1, 0.2]), (nseq, frames, 3)).copy()

    def step(self, n):
        self.steps += n

    def position_log(self, seq0=0, nseq=None, capacity=1000):
        nseq = self.nseq - seq0 if nseq is None else nseq
        n = min(capacity, self.steps, 1000)
        return self.truth(self.nseq, self.steps)[seq0:seq0 + nseq, self.steps - n:]


@pytest.mark.parametrize("warmup,timed", [(30, 100), (30, 1332), (5, 2000), (0, 1500), (1200, 300)])
def test_oracle_legs_compare_the_frames_the_engine_still_holds(warmup, timed):
    """A --full run of more than 1000 stepped frames: the legs compare the oracle with the engine on the frames the engine's
    log still holds (the warm-up's, read before the timed steps, and the last 1000), never on positions of other frames."""
    import bench
    eng = _Logging(6)
    eng.step(warmup)
    head = (eng.position_log(0, None, capacity=bench.POS_LOG), warmup) if warmup else None
    eng.step(timed + 4)
    stepped = warmup + timed + 4
    for nseq, frames in ((2, 8), (4, 25), (3, stepped), (3, min(stepped, 1100))):
        pos = bench.held_positions(eng, nseq, head, stepped, frames)
        want = _Logging.truth(nseq, frames)
        held = np.isfinite(pos).all(axis=(0, 2))
        k = np.arange(1, frames + 1)                 # held: the last 1000 frames of the warm-up and of the whole run
        expect = ((k > warmup - 1000) & (k <= warmup)) | (k > stepped - 1000)
        assert np.array_equal(held, expect), (nseq, frames)
        assert np.array_equal(pos[:, held], want[:, held])
        rmse, maxabs, compared = bench.compare_positions(pos, want)
        assert compared == held.sum()
        if compared:
            assert rmse == 0.0 and maxabs == 0.0
            off = want.copy()
            off[:, held.argmax(), 1] += 1e-3
            assert bench.compare_positions(pos, off)[1] == pytest.approx(1e-3)
        else:
            assert rmse is None and maxabs is None
