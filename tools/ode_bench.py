"""Fixed-grid ODE solvers at an equal number of network evaluations on configs1's shape (engine option "ode_method").

    python tools/ode_bench.py [--evals 32] [--reps 5] [--kernel-stats DIR] [--out profiles/ode_methods.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/ode_bench.py --profile-run rk4     (one method per profiler run)

Full depth, B = 1, prompt F = 938, N = 1875 frames, CFG 2, sway 5, SYNTHETIC weights (lemas_tts_amd.synth, seed 1234) -- the same inputs
for every method: euler at E steps, midpoint at E / 2, rk4 at E / 4 (E network evaluations each).  Per method: the sampler's throughput in
generated audio-seconds per second (the DiT solve of CFM.sample: prepare + solve, no vocoder), the solve's ms per network evaluation
(prepare / solve split, CUDA events), the update kernel's share of the solve from a rocprofv3 --kernel-trace --stats run (--kernel-stats:
the directories of the --profile-run passes), and the mel distance (RMS over the generated frames) to a fine solve of the same inputs
(rk4, 64 steps = 256 evaluations).  Quality per cost on synthetic weights: the distances rank the solvers on this flow only; they say
nothing about speech quality of a trained checkpoint."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lemas_tts_amd import synth  # noqa: E402
from lemas_tts_amd.model.cfm import CFM, ODE_STAGES  # noqa: E402
from lemas_tts_amd.model.layout import DiTArch  # noqa: E402

VOCAB, F_REF, N_TOT, NT, CFG, SWAY, HOP, SR = 898, 938, 1875, 319, 2.0, 5, 256, 24000
UPDATE_KERNEL = {"euler": "cfg_euler_kernel", "midpoint": "ode_stage_kernel", "rk4": "ode_stage_kernel"}


def build():
    arch = DiTArch()
    sd = synth.synth_cfm_state_dict(arch, VOCAB, 1234)
    model = CFM(arch, VOCAB, sd, device="cuda:0")
    cond = torch.from_numpy(synth.synth_cond_mel(1235, F_REF))[None]
    text = torch.from_numpy(np.asarray(synth.synth_tokens(1236, NT, VOCAB), dtype=np.int64))[None]
    y0 = torch.from_numpy(synth.synth_noise(1237, N_TOT))[None]
    return model, cond, text, y0


def sample(model, inp, method, steps):
    cond, text, y0 = inp
    model.odeint_kwargs = dict(method=method)
    out, _ = model.sample(cond, text, N_TOT, steps=steps, cfg_strength=CFG, sway_sampling_coef=SWAY, y0=y0, use_acc_grl=False)
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), r


def kernel_share(stats_dir, kernel):
    """(update-kernel total ns, its calls, all kernels' total ns) from a rocprofv3 --stats kernel_stats.csv under stats_dir"""
    files = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    tot, mine, calls = 0.0, 0.0, 0
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            ns = float(row["TotalDurationNs"])
            tot += ns
            if kernel + "(" in row["Name"]:
                mine += ns
                calls += int(row["Calls"])
    return mine, calls, tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-run", default=None, help="one method, a few solves: the pass to run under rocprofv3")
    ap.add_argument("--kernel-stats", nargs="*", default=[], help="method=DIR of a --profile-run pass under rocprofv3 --stats")
    ap.add_argument("--lease", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model, cond, text, y0 = build()
    inp = (cond, text, y0)
    if a.profile_run:
        m = a.profile_run
        for _ in range(3):
            sample(model, inp, m, a.evals // ODE_STAGES[m])
        torch.cuda.synchronize()
        return
    stats = dict(s.split("=", 1) for s in a.kernel_stats)
    fine = sample(model, inp, "rk4", 64).cpu().numpy()[0, F_REF:]
    rows = []
    for m in ("euler", "midpoint", "rk4"):
        steps = a.evals // ODE_STAGES[m]
        E = steps * ODE_STAGES[m]
        sample(model, inp, m, steps)                                   # warm-up: tables, graph capture
        torch.cuda.synchronize()
        ms_sample, out = timed(lambda: sample(model, inp, m, steps), a.reps)
        call = model.last_engine_call
        eng = model.engine
        eng.prepare(call["cond"], call["cond_mask"], call["text"], call["t_grid"], cond_frames=call["cond_frames"],
                    cfg_strength=call["cfg_strength"], seq_len=call["seq_len"], prosody=call["prosody"])
        eng.solve(call["y0"])
        ms_solve, _ = timed(lambda: eng.solve(call["y0"]), a.reps)
        gen = out.cpu().numpy()[0, F_REF:]
        audio = (N_TOT - F_REF) * HOP / SR
        row = {"method": m, "steps": steps, "evaluations": E, "sample_ms": ms_sample, "audio_s_per_s": audio / (ms_sample * 1e-3),
               "solve_ms": ms_solve, "ms_per_evaluation": ms_solve / E,
               "rms_to_fine_solve": float(np.sqrt(((gen - fine) ** 2).mean()))}
        if m in stats:
            ks = kernel_share(stats[m], UPDATE_KERNEL[m])
            if ks:
                row.update(update_kernel=UPDATE_KERNEL[m], update_kernel_us_per_launch=ks[0] / max(ks[1], 1) / 1e3,
                           update_kernel_share_of_gpu_time=ks[0] / ks[2])
        rows.append(row)
    base = rows[0]["ms_per_evaluation"]
    for r in rows:
        r["ms_per_evaluation_vs_euler"] = r["ms_per_evaluation"] / base - 1.0
    res = {"what": "fixed-grid ODE solvers at equal network evaluations, configs1 shape (B 1, F 938, N 1875, full depth, CFG 2, sway 5); "
                   "SYNTHETIC weights: rms_to_fine_solve ranks solvers on this flow only (fine solve: rk4, 64 steps)",
           "lease": a.lease, "evaluations": a.evals, "reps": a.reps, "time": time.strftime("%Y-%m-%d %H:%M:%S"), "rows": rows}
    print(json.dumps(res, indent=1))
    print(f"{'method':9s} {'steps':>5s} {'E':>4s} {'audio-s/s':>10s} {'ms/eval':>8s} {'vs euler':>9s} {'upd us':>7s} {'upd share':>9s} {'rms to fine':>11s}")
    for r in rows:
        print(f"{r['method']:9s} {r['steps']:5d} {r['evaluations']:4d} {r['audio_s_per_s']:10.1f} {r['ms_per_evaluation']:8.3f} "
              f"{100 * r['ms_per_evaluation_vs_euler']:+8.2f}% {r.get('update_kernel_us_per_launch', float('nan')):7.2f} "
              f"{100 * r.get('update_kernel_share_of_gpu_time', float('nan')):8.3f}% {r['rms_to_fine_solve']:11.3e}")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
