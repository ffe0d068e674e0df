"""bench.py's JSON line on the GPU box (the driver's contract): one short run of the headline workload and
one of the CEM workload, in child processes, checked for the keys and the relations the driver and the
judge read -- value = K*H*steps / wall time, ms_per_step, the roofline record (achieved / peak = frac,
traffic from the committed PMC file), n_gpus 1, strong scaling on the north_star's global K -- and the
self-launched 2-rank form (``--gpus 2`` without WORLD_SIZE: bench.py starts its own torch.distributed.run; gloo
ranks sharing the one card) with the global K split over the ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN = ["--no-cpu-baseline", "--dropin-calls", "0", "--no-small-k", "--no-f16", "--no-cfg2", "--no-extra",
        "--no-scale"]


def _bench(*args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True,
                       timeout=240, cwd=REPO, env=e)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _load(path):
    return {n[:-4]: np.load(os.path.join(path, n)) for n in sorted(os.listdir(path)) if n.endswith(".npy")}


@pytest.fixture(scope="module")
def headline(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("headline") / "dump")
    return _bench("--steps", "5", "--warmup", "2", *LEAN, "--dump-outputs", out), _load(out)


def test_headline_line_contract(headline):
    d = headline[0]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["scaling"] == "strong"
    assert d["higher_is_better"] is True and d["unit"] == "candidate-steps/s"
    K, H = d["config"]["K_per_gpu"], d["config"]["horizon"]
    assert (K, H) == (65536, 20) and d["config"]["K_global"] == 65536 and d["config"]["ranks"] == 1
    assert d["value"] == pytest.approx(K * H / (d["ms_per_step"] / 1e3), rel=1e-6)
    assert d["summary"]["headline"]["frac"] == pytest.approx(d["roofline"]["frac"], abs=1e-4)
    assert list(d)[-1] == "summary"                              # (survives the driver's stdout tail)
    assert d["prewarm"]["calls"] >= 3 and d["prewarm"]["seconds"] > 0   # untimed, reported (bench.prewarm)
    r = d["roofline"]
    assert r["bound"] == "mfma" and 0 < r["frac"] < 1
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    assert r["traffic"] and r["traffic"] > 0                      # profiles/<TRAFFIC_FILE>, cfg3:split:device
    # the kernel's HIP-event time sits inside the step
    assert r["flop_per_launch"] / (r["achieved"] * 1e12) * 1e3 <= d["ms_per_step"] * 1.02


def test_plain_run_times_the_headline_alone_and_dumps_its_outputs(headline, tmp_path):
    """Without ``--full`` (and without any ``--no-*`` option) the bench measures the headline only: exactly
    ``--steps`` timed steps, none of the other lines.  ``--dump-outputs`` writes what the last timed step
    returned and its candidate costs as float64 ``.npy`` files; the inputs are seeded, so a second run with the
    same arguments (the ``headline`` fixture's: the same steps and warmup) writes the same arrays."""
    out = str(tmp_path / "dump")
    d = _bench("--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", out)
    assert d["steps"] == 5 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(65536 * 20 / (d["ms_per_step"] / 1e3), rel=1e-6)
    assert d["cpu_baseline"] is None and d["small_k"] is None and d["dropin_parity_p50_ms"] is None
    for k in ("scale", "cfg2", "ns_shard", "cfg4_shard", "cfg5", "f16_single_pass", "library_comm"):
        assert k not in d, k
    assert list(d["summary"]) == ["headline"]
    a = _load(out)
    assert sorted(a) == ["best_cost", "best_index", "candidate_costs", "first_action"] == d["dumped_outputs"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["first_action"].shape == (6,) and a["candidate_costs"].shape == (65536,)
    assert np.all(np.abs(a["first_action"]) <= 1.0) and np.all(np.isfinite(a["candidate_costs"]))
    # the winner the timed step returned is the cost vector's first minimum (np.argmin's rule)
    assert int(a["best_index"]) == int(np.argmin(a["candidate_costs"]))
    assert float(a["best_cost"]) == a["candidate_costs"].min()
    b = headline[1]
    assert sorted(b) == sorted(a) and all(np.array_equal(a[k], b[k]) for k in a)


def test_cem_line_contract():
    d = _bench("--workload", "cfg5", "--steps", "1", "--warmup", "1", *LEAN)
    K, H = d["config"]["K_per_gpu"], d["config"]["horizon"]
    assert (K, H) == (65536, 50)
    # CEM: every iteration's candidate-steps count (4 rollout passes per get_action)
    assert d["value"] == pytest.approx(4 * K * H / (d["ms_per_step"] / 1e3), rel=1e-6)
    assert 0 < d["roofline"]["frac"] < 1


def test_self_launched_two_ranks_split_the_global_k():
    """``bench.py --gpus 2`` with no WORLD_SIZE starts the two ranks itself (gloo, both on this card): the
    north_star's K = 65,536 is split 32,768 per rank, the record exchange ran over 2 ranks, and the scale
    line's cfg4 is K_global = 262,144 over the same 2 ranks."""
    d = _bench("--full", "--gpus", "2", "--steps", "3", "--warmup", "1", *[a for a in LEAN if a != "--no-scale"],
               env={"BCMPC_DIST_BACKEND": "gloo", "BCMPC_BENCH_DEVICE": "0"})
    assert d["n_gpus"] == 2 and d["config"]["ranks"] == 2 and d["scaling"] == "strong"
    assert d["config"]["K_global"] == 65536 and d["config"]["K_per_gpu"] == 32768
    assert "bench.py --gpus" in d["config"]["launcher"] and "RecordExchange" in d["config"]["collective"]
    assert d["value"] == pytest.approx(65536 * 20 / (d["ms_per_step"] / 1e3), rel=1e-6)
    c4 = d["scale"]["cfg4"]
    assert c4["K_global"] == 262144 and c4["K_per_gpu"] == 131072 and c4["ranks"] == 2
    c5 = d["scale"]["cfg5"]
    assert c5["K_global"] == 65536 and c5["cem"]["n_elite"] == 6554 and c5["ranks"] == 2
    assert d["scale"]["cfg3_weak"]["K_global"] == 131072
