"""GPU: a plain `bench.py` run (no --full) at a tiny size.

* It times exactly --steps proofs, verifies them, reports `ms_per_step` consistently with `value`, and runs none of
  the secondary legs (their keys are null), whatever the legs' own switches say.
* `--dump-outputs DIR` writes the last timed step's proof as DIR/proofs.npy (float32, one value per byte).  The
  bench's inputs all come from fixed seeds, so the same proof is computed here, in this process, from the same
  circuit, key, witness and blinding pair, and the dumped bytes must equal it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_ROWS, STEPS, WARMUP = 12, 3, 1


def test_bench_plain_run_is_lean_and_dumps_last_step_proof(ctx, tmp_path):
    import bench
    import fil_groth16 as fg
    from fil_groth16 import synth

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--log-rows", str(LOG_ROWS), "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["full"] is False and out["steps"] == STEPS and out["warmup"] == WARMUP and out["n_gpus"] == 1
    assert out["verified"] and out["verified_proofs"] == STEPS
    assert out["unit"] == "constraints/s" and out["higher_is_better"] is True
    n = out["config"]["constraints"]
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(n / (out["ms_per_step"] * 1e-3), rel=1e-9)
    for leg in ("device_resident", "msm_g1_mpoints_per_s", "cpu_baseline", "tree_c", "sdr_labels", "uniform_witness",
                "config4", "config5", "stacked_porep_32gib", "window_post_32gib", "winning_post_32gib"):
        assert out[leg] is None, leg
    assert out["config2_micro"] == {} and out["valu_roofline"]["one_lane"] is None
    assert out["setup_s"]["params_load"] is None
    assert os.listdir(dump) == ["proofs.npy"]
    got = np.load(dump / "proofs.npy")
    assert got.dtype == np.float32 and got.shape == (1, 192)
    assert np.array_equal(got, np.floor(got)) and got.min() >= 0 and got.max() <= 255

    # the last timed step's proof, recomputed from the bench's seeds
    sc = synth.SynthCircuit(LOG_ROWS, 4, 1)
    assert sc.n == n
    circ = sc.load(ctx)
    pk = fg.generate_random_parameters(ctx, circ, bench.splitmix_frs(bench.TOXIC_SEED, 5))
    blind = bench.splitmix_frs(1000, 2 * (WARMUP + STEPS))
    last = WARMUP + STEPS - 1
    z = fg.HostBuffer(32 * sc.num_vars)
    np.copyto(z.array, sc.z_array())
    want = fg.prove_batch(ctx, pk, circ, [z], [(blind[2 * last], blind[2 * last + 1])])[0]
    assert got.astype(np.uint8).tobytes() == want
    del pk, circ, z, sc
