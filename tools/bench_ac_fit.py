"""Time the actor-critic fitter (csrc/ac_fit.hip) at the reference shape and write profiles/ac_fit.json.

ppo_bc_policy.py / train_mpc_ppo.py:358-372: 500 Adam steps (optim_epochs) of batch 128 per on-policy iteration on
the 20 -> 128 -> 128 -> 6 tanh policy (BC loss) and the 20 -> 128 -> 128 -> 1 critic.  Per head and batch size
(128, 64): us per step and ms per 500-step epoch on the graph path and on the per-step launch path (median of
``--reps`` epochs after a warm-up epoch, wall time around ``run`` with the indices already drawn), and the
definition's (bc_mpc_amd/ac_fit.py, NumPy) time per step on the host's BLAS threads.  ``--kernels CSV`` (the
kernel-stats file of a ``rocprofv3 --kernel-trace --stats --output-format csv`` run of this script) runs nothing:
it adds the two kernels' mean times to the existing ``--out`` file.

usage: python tools/bench_ac_fit.py [--steps 500] [--reps 7] [--cpu-steps 50] [--out profiles/ac_fit.json]
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def kernel_times(path):
    """{kernel name: mean us} of the acfit kernels in a kernel-stats CSV (Name, ..., AverageNs columns)."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            if "acfit_" in name:
                ns = row.get("AverageNs") or row.get("Average") or row.get("AVG_NS")
                out[name.split("(")[0].split("::")[-1]] = float(ns) / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-steps", type=int, default=50)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ac_fit.json"))
    args = ap.parse_args()
    if args.kernels:
        with open(args.out) as fh:
            doc = json.load(fh)
        doc["kernel_mean_us"] = kernel_times(args.kernels)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        return
    import torch  # noqa: F401  (single HIP runtime)
    from bc_mpc_amd import ac_fit
    from oracle import mpc_oracle as orc
    S, A, h, L, lr = 20, 6, 128, 2, 1e-3
    rs = np.random.RandomState(5)
    results = []
    for head in ("policy", "value"):
        out = A if head == "policy" else 1
        w = orc.synthetic_policy(S, out, h, L)
        obs = w.ob_mean.astype(np.float64) + 1.5 * w.ob_std.astype(np.float64) * rs.standard_normal((args.rows, S))
        tgt = rs.uniform(-1, 1, (args.rows, out)) if head == "policy" else 3.0 * rs.standard_normal((args.rows, 1))
        params = []
        for k, b in zip(w.kernels, w.biases):
            params += [k, b]
        for B in (128, 64):
            batches = [rs.choice(args.rows, B, replace=False) for _ in range(args.steps)]
            rec = {"head": head, "shape": f"{S}->{h}x{L}->{out} tanh", "batch": B, "steps": args.steps}
            for path, env in (("graph", "1"), ("launch", "0")):
                os.environ["BCMPC_ACFIT_GRAPH"] = env
                f = ac_fit.ActorCriticFitter(head, S, out, h, L, batch_size=B)
                f.set_params(params[0::2], params[1::2])
                f.set_filter(w.ob_mean, w.ob_std)
                f.set_data(obs, tgt)
                f.run(batches, lr)                                # warm-up (and the capture)
                times = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    f.run(batches, lr)
                    times.append(time.perf_counter() - t0)
                assert (f.graph_captures == 1) == (path == "graph")
                f.close()
                med = float(np.median(times))
                rec[f"{path}_us_per_step"] = med / args.steps * 1e6
                rec[f"{path}_ms_per_epoch"] = med * 1e3
                rec[f"{path}_ms_per_epoch_min_max"] = [min(times) * 1e3, max(times) * 1e3]
            os.environ.pop("BCMPC_ACFIT_GRAPH", None)
            ps = [p.copy() for p in params]
            st = ac_fit.AdamState.zeros_like(ps)
            ac_fit.run(ps, st, head, (w.ob_mean, w.ob_std), obs, tgt, batches[:5], lr)
            t0 = time.perf_counter()
            ac_fit.run(ps, st, head, (w.ob_mean, w.ob_std), obs, tgt, batches[:args.cpu_steps], lr)
            rec["definition_us_per_step"] = (time.perf_counter() - t0) / args.cpu_steps * 1e6
            rec["definition_threads"] = os.environ.get("OMP_NUM_THREADS", "default")
            dims = [S] + [h] * L + [out]
            mac = sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
            rec["flop_per_step"] = 3 * 2 * mac * B                # forward + two backward GEMMs per layer
            results.append(rec)
            print(json.dumps(rec))
    doc = {"metric": "actor-critic fitter: BC distillation / critic regression step time", "reps": args.reps,
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
