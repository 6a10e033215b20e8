"""Golden vectors for the higher-order fixed-grid ODE solvers (``odeint_kwargs=dict(method=...)``) by RUNNING THE REFERENCE.

    python tools/gen_golden_ode.py            # build container only (needs the reference tree); writes tests/golden/*.npz

The reference solves with ``odeint(fn, y0, t, **self.odeint_kwargs)`` (cfm.py:456) from torchdiffeq, which is not installed
here.  ``oracle/ref_shims.py`` restates its Euler step only; this script installs those shims unchanged, then replaces the
``odeint`` the reference's cfm module imported (``from torchdiffeq import odeint``) by :func:`odeint_fixed_grid` below, a
restatement of torchdiffeq 0.2.4's fixed-grid solvers, and sets the reference CFM's ``odeint_kwargs`` to the method.  The
cases reuse ``oracle.gen_golden.run_case``: same inputs, same layout as the ``mini_*`` / ``full_*`` fixtures, plus an
``ode_method`` code (1 = midpoint, 2 = rk4).  Only numeric arrays are written.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden, ref_shims  # noqa: E402

METHOD_CODE = {"euler": 0, "midpoint": 1, "rk4": 2}


def odeint_fixed_grid(func, y0, t, method="euler", **_):
    """torchdiffeq 0.2.4 ``odeint`` with a fixed-grid method and output times equal to the grid (``FixedGridODESolver.integrate``:
    dt = t1 - t0 in the grid's dtype, y1 = y0 + dy; ``_linear_interp`` returns y1 exactly at t == t1), fp32 throughout:
      euler     dy = dt * f(t0, y0)
      midpoint  half_dt = 0.5 * dt;  f0 = f(t0, y0);  y_mid = y0 + f0 * half_dt;  dy = dt * f(t0 + half_dt, y_mid)
      rk4       (rk_common.rk4_alt_step_func, the 3/8 rule)
                k1 = f(t0, y0)
                k2 = f(t0 + dt * (1/3), y0 + dt * k1 * (1/3))
                k3 = f(t0 + dt * (2/3), y0 + dt * (k2 - k1 * (1/3)))
                k4 = f(t1, y0 + dt * (k1 - k2 + k3))
                dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
    The solution holds one row per STEP (stages are not stored)."""
    if method not in METHOD_CODE:
        raise NotImplementedError(f"fixed-grid methods only: {sorted(METHOD_CODE)}")
    assert bool((t[1:] > t[:-1]).all()), "t must be strictly increasing"
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    sol = [y0]
    y = y0
    for k in range(t.shape[0] - 1):
        t0, t1 = t[k].to(y.dtype), t[k + 1].to(y.dtype)
        dt = t1 - t0
        if method == "euler":
            dy = dt * func(t0, y)
        elif method == "midpoint":
            half_dt = 0.5 * dt
            f0 = func(t0, y)
            y_mid = y + f0 * half_dt
            dy = dt * func(t0 + half_dt, y_mid)
        else:
            k1 = func(t0, y)
            k2 = func(t0 + dt * third, y + dt * k1 * third)
            k3 = func(t0 + dt * two_thirds, y + dt * (k2 - k1 * third))
            k4 = func(t1, y + dt * (k1 - k2 + k3))
            dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        y = y + dy
        sol.append(y)
    return torch.stack(sol, dim=0)


_method = {"name": "euler"}


def _install():
    ref_shims.install()
    import lemas_tts.model.cfm as ref_cfm            # the reference module: its module-level `odeint` is what cfm.py:456 calls
    ref_cfm.odeint = odeint_fixed_grid
    sys.modules["torchdiffeq"].odeint = odeint_fixed_grid
    build = ref_shims.build_reference_cfm

    def build_with_method(*a, **k):
        cfm = build(*a, **k)
        cfm.odeint_kwargs = dict(method=_method["name"])
        return cfm

    gen_golden.ref_shims.build_reference_cfm = build_with_method


def run(name, method, arch, **kw):
    _method["name"] = method
    gen_golden.run_case(name, arch, **kw)
    path = os.path.join(gen_golden.GOLDEN, name + ".npz")
    fx = dict(np.load(path))
    fx["ode_method"] = np.int64(METHOD_CODE[method])
    np.savez_compressed(path, **fx)


def main():
    torch.set_num_threads(8)
    _install()
    MINI, FULL = gen_golden.MINI, gen_golden.FULL
    # the inputs of mini_plain / mini_batch / mini_nocfg_nosway / full_plain, fewer steps (each costs 2 or 4 network evaluations)
    run("mini_midpoint", "midpoint", MINI, wseed=11, B=1, F=60, lens=None, Nt=[30], duration=160, steps=4, cfg=2.0, coef=5, noise_seed=101)
    run("mini_rk4", "rk4", MINI, wseed=11, B=1, F=60, lens=None, Nt=[30], duration=160, steps=3, cfg=2.0, coef=5, noise_seed=101)
    run("mini_batch_midpoint", "midpoint", MINI, wseed=13, B=2, F=70, lens=[50, 70], Nt=[24, 31], duration=[120, 150], steps=3,
        cfg=2.0, coef=5, noise_seed=103)
    run("mini_rk4_nocfg", "rk4", MINI, wseed=12, B=1, F=40, lens=None, Nt=[20], duration=96, steps=2, cfg=0.0, coef=None,
        noise_seed=102)
    run("full_midpoint", "midpoint", FULL, wseed=16, B=1, F=150, lens=None, Nt=[60], duration=400, steps=2, cfg=2.0, coef=5,
        noise_seed=106)


if __name__ == "__main__":
    main()
