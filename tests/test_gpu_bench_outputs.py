"""bench.py's plain run, --full and --dump-outputs.

* dump_outputs writes, per level, exactly the chunk layers the last step
  completed (oracle-exact; whole layers when small, else the seeded sample
  of their positions) and their has_data flags, as float32.
* A plain `bench.py --gpus 1 --steps N --warmup W` line holds the headline
  fields and none of the side measurements; two runs with the same arguments
  dump identical arrays; --full adds the side measurements to the line.

The command-line runs use C1 at 64-frame launches (512x512 u16 frames, the
smallest configuration) so each takes a few seconds.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from helpers import expected_stage_layers
from oracle_bindings import MEAN, SPACE, TIME, U16, synthetic_frames

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--config", "c1", "--batch", "64", "--steps", "3", "--warmup", "1"]
SIDE_KEYS = ("pyramid_only", "hbm_probe", "cpu_baseline")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
                        *SMALL, *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dump_a"))
    return _bench("--dump-outputs", d), _load(d)


def test_dump_outputs_is_the_last_steps_layers(gpu, tmp_path, monkeypatch):
    """Two launches of 4 frames at t-chunk 2: the last one completes layers
    2 and 3 of every level; a 4-slot ring still holds them."""
    dims = [(TIME, 0, 2, 1), (SPACE, 300, 64, 1), (SPACE, 260, 64, 1)]
    frames = synthetic_frames(U16, 8, 300, 260, 23)
    exp, fw, _ = expected_stage_layers(dims, U16, MEAN, frames)
    st = gpu.Stage(dims, U16, MEAN, layer_slots=4, max_batch_frames=4)
    L = st.n_levels()
    assert L > 1 and fw == [8] * L
    st.append(frames[:4])
    st.append(frames[4:])
    st.synchronize()
    after = [st.frames_written(l) for l in range(L)]
    assert after == fw
    before = [4] * L
    whole, sampled = str(tmp_path / "whole"), str(tmp_path / "sampled")
    bench.dump_outputs(st, {"dtype": U16}, whole, before, after)
    share = 1000
    monkeypatch.setattr(bench, "DUMP_VALUES", share * L * 2)
    bench.dump_outputs(st, {"dtype": U16}, sampled, before, after)
    st.close()
    got, gots = _load(whole), _load(sampled)
    assert sorted(got) == sorted(gots) == sorted(
        f"level{l}{s}.npy" for l in range(L) for s in ("", "_has_data"))
    for l in range(L):
        px = [exp[(l, k)][0].view(np.uint16) for k in (2, 3)]
        flags = np.concatenate([exp[(l, k)][1] for k in (2, 3)])
        for g in (got, gots):
            assert g[f"level{l}.npy"].dtype == g[f"level{l}_has_data.npy"].dtype == np.float32
            assert np.array_equal(g[f"level{l}_has_data.npy"], flags)
        assert np.array_equal(got[f"level{l}.npy"], np.concatenate(px))
        want = []
        for i, p in enumerate(px):
            if p.size > share:
                rng = np.random.default_rng([bench.DUMP_SEED, l, i, p.size])
                p = p[np.sort(rng.integers(0, p.size, size=share))]
            want.append(p)
        assert np.array_equal(gots[f"level{l}.npy"], np.concatenate(want))
    # level 0's layers are larger than the share: the sample was exercised
    assert gots["level0.npy"].size == 2 * share < got["level0.npy"].size


def test_plain_line_is_lean_and_dumps_every_level(plain_run):
    line, dump = plain_run
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u16" and line["metric"].startswith("input GB/s")
    # value and ms_per_step describe the same timed steps
    fbytes = 512 * 512 * 2
    assert line["value"] == pytest.approx(64 * fbytes / (line["ms_per_step"] * 1e-3) / 1e9,
                                          rel=1e-3)
    assert not [k for k in SIDE_KEYS if k in line]
    assert line["roofline"]["traffic"] is None
    levels = line["config"]["levels"]
    assert sorted(dump) == sorted(f"level{l}{s}.npy" for l in range(levels)
                                  for s in ("", "_has_data"))
    assert sum(a.nbytes for a in dump.values()) <= 64 << 20
    for l in range(levels):
        a = dump[f"level{l}.npy"]
        assert a.dtype == np.float32 and a.size > 0 and a.max() > 0
        # one 64-frame launch = one chunk layer (t-chunk 64) of every level
        side = 512 >> l
        assert a.size == min(64 * side * side, bench.DUMP_VALUES // levels)
        assert np.all(dump[f"level{l}_has_data.npy"] == 1)


def test_same_arguments_dump_the_same_outputs(plain_run, tmp_path):
    _, first = plain_run
    _bench("--dump-outputs", str(tmp_path))
    second = _load(str(tmp_path))
    assert sorted(first) == sorted(second)
    for name in first:
        assert np.array_equal(first[name], second[name]), name


def test_full_adds_the_side_measurements():
    line = _bench("--full", "--cpu-seconds", "0.5")
    assert all(k in line for k in SIDE_KEYS)
    assert line["pyramid_only"]["value"] > 0 and line["hbm_probe"]["read_gbs"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert line["steps"] == 3 and line["ms_per_step"] > 0
