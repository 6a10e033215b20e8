"""CPU tier: the fixed-grid midpoint / rk4 solvers (``odeint_kwargs=dict(method=...)``, engine option "ode_method").

The fixtures tests/golden/{mini_midpoint, mini_rk4, mini_batch_midpoint, mini_rk4_nocfg, full_midpoint}.npz are the reference's own
``CFM.sample`` with ``odeint`` replaced by a restatement of torchdiffeq 0.2.4's fixed-grid solvers (tools/gen_golden_ode.py).  Here the
fp32 oracle's solver is swapped for a test-local restatement of the same arithmetic and must reproduce them at fp32 round-off; the public
entry points must refuse every other method; the host evaluation grid is pinned against the formulas."""
import os

import numpy as np
import pytest
import torch

from lemas_tts_amd import synth
from lemas_tts_amd.model.layout import DiTArch
from oracle import lemas_oracle as O

CASES = ["mini_midpoint", "mini_rk4", "mini_batch_midpoint", "mini_rk4_nocfg", "full_midpoint"]
METHOD = {1: "midpoint", 2: "rk4"}
ATOL = 5e-5     # as tests/test_oracle_golden.py: fp32 on both sides, only the summation order of the network differs


def fixed_grid_solve(method):
    """torchdiffeq 0.2.4 FixedGridODESolver.integrate with Midpoint / RK4 (rk4_alt_step_func), output times = the grid."""
    def solve(fn, y0, t):
        assert bool((t[1:] > t[:-1]).all())
        ys, y = [y0], y0
        for k in range(t.shape[0] - 1):
            t0, t1 = t[k], t[k + 1]
            dt = t1 - t0
            if method == "midpoint":
                half_dt = 0.5 * dt
                f0 = fn(t0, y)
                dy = dt * fn(t0 + half_dt, y + f0 * half_dt)
            else:
                k1 = fn(t0, y)
                k2 = fn(t0 + dt * (1 / 3), y + dt * k1 * (1 / 3))
                k3 = fn(t0 + dt * (2 / 3), y + dt * (k2 - k1 * (1 / 3)))
                k4 = fn(t1, y + dt * (k1 - k2 + k3))
                dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
            y = y + dy
            ys.append(y)
        return torch.stack(ys)
    return solve


def load_case(golden_dir, name):
    fx = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    arch = DiTArch(depth=int(fx["arch_depth"]))
    sd = synth.synth_cfm_state_dict(arch, int(fx["vocab"]), int(fx["wseed"]), prosody=bool(fx["prosody"]))
    assert abs(synth.checksum(sd) - float(fx["wchecksum"])) < 1e-6 * abs(float(fx["wchecksum"])), "RNG drift"
    return fx, arch, sd


@pytest.mark.parametrize("name", CASES)
def test_oracle_with_restated_solver_matches_reference_golden(golden_dir, name, monkeypatch):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    fx, arch, sd = load_case(golden_dir, name)
    method = METHOD[int(fx["ode_method"])]
    monkeypatch.setattr(O, "euler_solve", fixed_grid_solve(method))
    coef = None if np.isnan(fx["coef"]) else float(fx["coef"])
    if coef is not None and coef == int(coef):
        coef = int(coef)
    B, dur = int(fx["B"]), fx["duration"]
    out, traj = O.OracleCFM(sd, arch).sample(torch.from_numpy(fx["cond"]), torch.from_numpy(fx["text"]),
                                             int(dur[0]) if B == 1 else torch.from_numpy(dur), y0=torch.from_numpy(fx["y0"]),
                                             lens=torch.from_numpy(fx["lens"]), steps=int(fx["steps"]), cfg_strength=float(fx["cfg"]),
                                             sway_sampling_coef=coef)
    assert traj.shape[0] == int(fx["steps"]) + 1                 # one row per step, not per stage
    np.testing.assert_allclose(traj.numpy(), fx["trajectory"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(out.numpy(), fx["out"], atol=ATOL, rtol=0)


def test_the_fixtures_are_not_euler(golden_dir):
    """The same inputs with the Euler oracle land far from the midpoint fixture: the fixture really holds another solver."""
    fx, arch, sd = load_case(golden_dir, "mini_midpoint")
    out, _ = O.OracleCFM(sd, arch).sample(torch.from_numpy(fx["cond"]), torch.from_numpy(fx["text"]), int(fx["duration"][0]),
                                          y0=torch.from_numpy(fx["y0"]), lens=torch.from_numpy(fx["lens"]), steps=int(fx["steps"]),
                                          cfg_strength=float(fx["cfg"]), sway_sampling_coef=int(fx["coef"]))
    assert float(np.abs(out.numpy() - fx["out"]).max()) > 1e-2


@pytest.mark.parametrize("method", ["dopri5", "adams", "explicit_adams", "rk4_fixed", ""])
def test_public_entry_points_refuse_other_solvers(method):
    from lemas_tts_amd.api import TTS
    from lemas_tts_amd.infer.utils_infer import load_model
    from lemas_tts_amd.model.cfm import CFM, ode_method_code
    arch = DiTArch(depth=1)
    with pytest.raises(NotImplementedError, match="euler, midpoint, rk4"):
        ode_method_code(dict(method=method))
    with pytest.raises(NotImplementedError, match="euler, midpoint, rk4"):
        CFM(arch, 898, {}, device="cuda:0", odeint_kwargs=dict(method=method))
    with pytest.raises(NotImplementedError, match="euler, midpoint, rk4"):
        load_model(None, dict(dim=1024, depth=1, heads=16, ff_mult=2, text_dim=512, conv_layers=4), "", ode_method=method,
                   device="cuda:0", state_dict={}, vocab_char_map={"a": 0})
    with pytest.raises(NotImplementedError, match="euler, midpoint, rk4"):
        TTS(ode_method=method, device="cuda:0", state_dict={}, vocoder_state_dict={}, vocab_char_map={"a": 0})


def test_supported_codes():
    from lemas_tts_amd.model.cfm import ode_method_code
    assert [ode_method_code(dict(method=m)) for m in ("euler", "midpoint", "rk4")] == [0, 1, 2]
    assert ode_method_code({}) == 0


def test_evaluation_grid_matches_the_formulas():
    from lemas_tts_amd.model.cfm import ode_eval_times, time_grid
    t = time_grid(5, 5)
    f32 = np.float32
    tn = t.numpy()
    np.testing.assert_array_equal(ode_eval_times(t, "euler").numpy(), tn[:-1])
    mid = ode_eval_times(t, "midpoint").numpy()
    rk4 = ode_eval_times(t, "rk4").numpy()
    assert mid.dtype == np.float32 and mid.shape == (10,) and rk4.shape == (20,)
    for k in range(5):
        t0, t1 = tn[k], tn[k + 1]
        dt = f32(t1 - t0)
        assert mid[2 * k] == t0 and mid[2 * k + 1] == f32(t0 + f32(f32(0.5) * dt))
        assert rk4[4 * k] == t0
        assert rk4[4 * k + 1] == f32(t0 + f32(dt * f32(1 / 3)))
        assert rk4[4 * k + 2] == f32(t0 + f32(dt * f32(2 / 3)))
        assert rk4[4 * k + 3] == t1            # k4 is evaluated at t1 itself, not at t0 + dt
    # stage times increase inside a step; rk4's last stage and the next step's first share t1
    assert (np.diff(mid) > 0).all() and (np.diff(rk4.reshape(5, 4), axis=1) > 0).all() and (np.diff(rk4) >= 0).all()
