"""GPU tier: the fixed-grid midpoint / rk4 solvers on the device step loop (engine option "ode_method", CFM odeint_kwargs["method"]).

Reference parity on the fixtures tools/gen_golden_ode.py wrote from the reference's own CFM.sample; the device solve against the same
solver composed on the host from single forwards (DiTEngine.forward at every evaluation); graph / eager and dual / single lane bit
identity; switching methods on one engine; Euler untouched; ragged batches with and without skip_masked; the public API end to end."""
import os

import numpy as np
import pytest
import torch

from lemas_tts_amd import synth
from lemas_tts_amd.model.layout import DiTArch

pytestmark = pytest.mark.gpu

MSE_TOL = 1e-4
METHOD = {0: "euler", 1: "midpoint", 2: "rk4"}
CASES = ["mini_midpoint", "mini_rk4", "mini_batch_midpoint", "mini_rk4_nocfg", "full_midpoint"]


def _load(golden_dir, name):
    fx = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    arch = DiTArch(depth=int(fx["arch_depth"]))
    sd = synth.synth_cfm_state_dict(arch, int(fx["vocab"]), int(fx["wseed"]), prosody=bool(fx["prosody"]))
    assert abs(synth.checksum(sd) - float(fx["wchecksum"])) < 1e-6 * abs(float(fx["wchecksum"])), "RNG drift"
    return fx, arch, sd


_models = {}


def _model(arch, fx, sd, method, fresh=False):
    from lemas_tts_amd.model.cfm import CFM
    key = (arch.depth, int(fx["wseed"]))
    if fresh:
        return CFM(arch, int(fx["vocab"]), sd, device="cuda:0", odeint_kwargs=dict(method=method))
    if key not in _models:
        _models.clear()  # one resident model at a time
        _models[key] = CFM(arch, int(fx["vocab"]), sd, device="cuda:0")
    m = _models[key]
    m.odeint_kwargs = dict(method=method)
    return m


def _coef(fx):
    coef = None if np.isnan(fx["coef"]) else float(fx["coef"])
    return int(coef) if coef is not None and coef == int(coef) else coef


def _run(m, fx, graph=True, traj=False):
    m.engine.set_option("graph", 1 if graph else 0)
    B, dur = int(fx["B"]), fx["duration"]
    out, tr = m.sample(torch.from_numpy(fx["cond"]), torch.from_numpy(fx["text"]), int(dur[0]) if B == 1 else torch.from_numpy(dur),
                       lens=torch.from_numpy(fx["lens"]), steps=int(fx["steps"]), cfg_strength=float(fx["cfg"]),
                       sway_sampling_coef=_coef(fx), y0=torch.from_numpy(fx["y0"]), return_trajectory=traj)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if tr is None else tr.cpu().numpy()


def _gen_mse(out, ref, fx):
    """MSE over the generated (non-conditioning) frames of every sample (tests/test_gpu_00_sample.py)."""
    se, cnt = 0.0, 0
    for b in range(int(fx["B"])):
        L, D = int(fx["lens"][b]), int(fx["duration"][b])
        keep = np.ones(out.shape[1], bool)
        keep[:L] = False
        keep &= np.arange(out.shape[1]) < D
        d = out[b, keep] - ref[b, keep]
        se += float((d.astype(np.float64) ** 2).sum())
        cnt += d.size
    return se / max(cnt, 1)


@pytest.mark.parametrize("name", CASES)
def test_solver_matches_reference_golden(golden_dir, name):
    fx, arch, sd = _load(golden_dir, name)
    m = _model(arch, fx, sd, METHOD[int(fx["ode_method"])])
    out, traj = _run(m, fx, graph=False, traj=True)
    mse = _gen_mse(out, fx["out"], fx)
    print(f"\n[{name}] mel-MSE {mse:.3e}  traj max|err| {np.abs(traj - fx['trajectory']).max():.3e}")
    assert traj.shape == fx["trajectory"].shape and traj.shape[0] == int(fx["steps"]) + 1      # one row per step, not per stage
    assert np.array_equal(traj[0], fx["y0"])
    assert mse <= MSE_TOL
    for k in range(1, traj.shape[0]):        # every step row, not only the end point
        assert _gen_mse(traj[k], fx["trajectory"][k], fx) <= MSE_TOL, k
    out_g, _ = _run(m, fx, graph=True)       # the graph path (one replay per evaluation) computes the same
    np.testing.assert_array_equal(out_g, out)


@pytest.mark.parametrize("name", ["mini_midpoint", "mini_rk4", "mini_rk4_nocfg"])
def test_solve_equals_the_solver_composed_from_single_forwards(golden_dir, name):
    """The device solve against torchdiffeq's arithmetic composed on the host in fp32 from DiTEngine.forward at every evaluation index,
    with CFG and the clamp on the host at the evaluation's time: a wrong stage time, CFG row, coefficient or base buffer shows far
    above the 1e-5 that FMA contraction inside the forward's own arithmetic leaves."""
    from lemas_tts_amd.model.cfm import ode_eval_times
    fx, arch, sd = _load(golden_dir, name)
    method = METHOD[int(fx["ode_method"])]
    m = _model(arch, fx, sd, method)
    _run(m, fx, graph=True)
    call = m.last_engine_call
    eng = m.engine
    eng.prepare(call["cond"], call["cond_mask"], call["text"], call["t_grid"], cond_frames=call["cond_frames"],
                cfg_strength=call["cfg_strength"], seq_len=call["seq_len"], prosody=call["prosody"])
    _, y_dev = eng.solve(call["y0"], want_out=False)
    y_dev = y_dev.cpu()
    t = torch.from_numpy(call["t_grid"])
    te = ode_eval_times(t, method)
    cfg = call["cfg_strength"]
    B = int(fx["B"])
    e = 0

    def f(x):
        nonlocal e
        pred = eng.forward(x, e).cpu()
        tt = te[e]
        e += 1
        if cfg < 1e-5:
            return pred
        pc, pu = pred[:B], pred[B:]
        return (pc + (pc - pu) * (cfg * (1 - tt) ** 2)).clamp(-20, 20)

    y = call["y0"].to(torch.float32).cpu()
    with pytest.raises(Exception, match="out of range|outside"):
        eng.forward(y, len(te))                               # the index is an evaluation index: [0, steps x stages)
    for k in range(t.shape[0] - 1):
        t0, t1 = t[k], t[k + 1]
        dt = t1 - t0
        if method == "midpoint":
            half_dt = 0.5 * dt
            f0 = f(y)
            dy = dt * f(y + f0 * half_dt)
        else:
            k1 = f(y)
            k2 = f(y + dt * k1 * (1 / 3))
            k3 = f(y + dt * (k2 - k1 * (1 / 3)))
            k4 = f(y + dt * (k1 - k2 + k3))
            dy = (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        y = y + dy
    assert e == len(te)
    diff = float((y - y_dev).abs().max())
    print(f"\n[{name}] composed vs solve max|diff| {diff:.3e}")
    assert diff <= 1e-5


@pytest.mark.parametrize("name", ["mini_midpoint", "mini_rk4", "mini_batch_midpoint"])
def test_graph_eager_and_lanes_are_bit_identical(golden_dir, name):
    fx, arch, sd = _load(golden_dir, name)
    m = _model(arch, fx, sd, METHOD[int(fx["ode_method"])])
    outs = {}
    for dual in (0, 1):
        m.engine.set_option("dual", dual)
        for graph in (False, True, True):
            outs.setdefault((dual, graph), []).append(_run(m, fx, graph=graph)[0])
    m.engine.set_option("dual", 1)
    ref = outs[(0, False)][0]
    for k, vs in outs.items():
        for v in vs:
            np.testing.assert_array_equal(v, ref, err_msg=str(k))


def test_switching_methods_on_one_engine(golden_dir):
    """euler -> midpoint -> rk4 -> euler on one engine and one input: each equals the same method on a fresh engine (table cache, graph
    cache and buffer sizes follow the method), the last Euler run equals the first."""
    fx, arch, sd = _load(golden_dir, "mini_midpoint")
    _models.clear()
    m = _model(arch, fx, sd, "euler")
    seq = ["euler", "midpoint", "rk4", "euler"]
    got = []
    for method in seq:
        m.odeint_kwargs = dict(method=method)
        got.append(_run(m, fx, graph=True)[0])
    np.testing.assert_array_equal(got[0], got[3])
    for method, g in zip(seq[:3], got[:3]):
        fresh = _model(arch, fx, sd, method, fresh=True)
        ref = _run(fresh, fx, graph=True)[0]
        fresh.engine.close()
        np.testing.assert_array_equal(g, ref, err_msg=method)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


def test_option_change_between_prepare_and_solve_is_refused(golden_dir):
    from lemas_tts_amd._lib import LemasError
    fx, arch, sd = _load(golden_dir, "mini_midpoint")
    m = _model(arch, fx, sd, "midpoint")
    ref = _run(m, fx, graph=True)[0]
    call = m.last_engine_call
    eng = m.engine
    kw = dict(cond_frames=call["cond_frames"], cfg_strength=call["cfg_strength"], seq_len=call["seq_len"], prosody=call["prosody"])
    eng.prepare(call["cond"], call["cond_mask"], call["text"], call["t_grid"], **kw)
    eng.set_option("ode_method", 1)                       # the same value: nothing changes
    eng.solve(call["y0"])
    eng.set_option("ode_method", 2)
    with pytest.raises(LemasError, match="code -10002"):  # LEMAS_E_STATE: prepare() must run again, never a stale solve
        eng.solve(call["y0"])
    with pytest.raises(LemasError, match="code -10002"):
        eng.forward(call["y0"], 0)
    eng.set_option("ode_method", 1)
    eng.prepare(call["cond"], call["cond_mask"], call["text"], call["t_grid"], **kw)
    out, _ = eng.solve(call["y0"])
    np.testing.assert_array_equal(out.cpu().numpy(), ref)
    with pytest.raises(LemasError, match="ode_method"):
        eng.set_option("ode_method", 3)


@pytest.mark.parametrize("name", ["mini_plain", "full_plain"])
def test_euler_is_untouched(golden_dir, name):
    """ode_method 0 set explicitly, and set back after another method, gives the default engine's Euler output bit for bit."""
    from lemas_tts_amd.model.cfm import CFM
    fx, arch, sd = _load(golden_dir, name)
    _models.clear()
    default = CFM(arch, int(fx["vocab"]), sd, device="cuda:0")
    ref = _run(default, fx, graph=True)[0]          # (CFM.sample sets "ode_method" 0: a repeat of the library's default is a no-op)
    default.engine.close()
    explicit = CFM(arch, int(fx["vocab"]), sd, device="cuda:0")
    explicit.engine.set_option("ode_method", 0)
    a = _run(explicit, fx, graph=True)[0]
    explicit.odeint_kwargs = dict(method="midpoint")
    mid = _run(explicit, fx, graph=True)[0]
    explicit.odeint_kwargs = dict(method="euler")
    b = _run(explicit, fx, graph=True)[0]
    c = _run(explicit, fx, graph=False)[0]
    explicit.engine.close()
    np.testing.assert_array_equal(a, ref)
    np.testing.assert_array_equal(b, ref)
    np.testing.assert_array_equal(c, ref)
    assert not np.array_equal(mid, ref)
    assert _gen_mse(ref, fx["out"], fx) <= MSE_TOL


def test_ragged_batch_skip_masked(golden_dir):
    fx, arch, sd = _load(golden_dir, "mini_batch_midpoint")
    m = _model(arch, fx, sd, "midpoint")
    outs = []
    for sm in (1, 0):
        m.engine.set_option("skip_masked", sm)
        outs.append(_run(m, fx, graph=True)[0])
    m.engine.set_option("skip_masked", 1)
    for o in outs:
        assert _gen_mse(o, fx["out"], fx) <= MSE_TOL
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize("method", ["midpoint", "rk4"])
def test_tts_and_infer_batch_process_end_to_end(method, monkeypatch):
    """TTS(ode_method=...) threads the method to its model; load_model(..., ode_method=...) + infer_batch_process synthesise against the
    oracle sampling the same utterance with the same solver (its Euler loop swapped for the host restatement)."""
    from test_ode_methods_cpu import fixed_grid_solve
    import lemas_tts_amd.api as A
    import lemas_tts_amd.infer.utils_infer as UI
    from lemas_tts_amd.infer.utils_infer import infer_batch_process, load_model, load_vocoder
    from oracle import lemas_oracle as O
    arch = DiTArch(depth=1)
    vocab = {f"p{i}": i for i in range(898)}
    sd = synth.synth_cfm_state_dict(arch, 898, 91)
    vsd = synth.synth_vocos_state_dict(92)
    _models.clear()
    cfg1 = lambda m: {**UI_load(m), "arch": {**UI_load(m)["arch"], "depth": 1}}
    UI_load = UI.load_arch_config
    monkeypatch.setattr(UI, "load_arch_config", cfg1)
    monkeypatch.setattr(A, "load_arch_config", cfg1)
    tts = A.TTS(model="multilingual_grl", ode_method=method, device="cuda:0", state_dict=sd, vocoder_state_dict=vsd, vocab_char_map=vocab)
    assert tts.ema_model.odeint_kwargs == dict(method=method)
    tts.ema_model.engine.close()
    model = load_model(None, dict(dim=1024, depth=1, heads=16, ff_mult=2, text_dim=512, conv_layers=4), "", ode_method=method,
                       device="cuda:0", state_dict=sd, vocab_char_map=vocab)
    vocoder = load_vocoder("vocos", device="cuda:0", state_dict=vsd)
    F_ = 50
    ref_mel = torch.from_numpy(synth.synth_cond_mel(93, F_))
    ref_text = [f"p{i}" for i in synth.synth_tokens(94, 10, 898)]
    gen = [[f"p{i}" for i in synth.synth_tokens(95, 8, 898)]]
    ref_len = F_ - 1
    dur = max(ref_len + int(ref_len / len(ref_text) * len(gen[0]) / 1.0), F_ + 1, len(ref_text) + len(gen[0]) + 1)
    noise = [torch.from_numpy(synth.synth_noise(96, dur))[None]]
    steps = 4 if method == "midpoint" else 2
    wav, sr, spec = next(infer_batch_process(ref_mel, ref_text, gen, model, vocoder, nfe_step=steps, cfg_strength=2.0,
                                             sway_sampling_coef=5, use_acc_grl=False, noise=noise))
    assert sr == 24000 and np.isfinite(wav).all()
    monkeypatch.setattr(O, "euler_solve", fixed_grid_solve(method))
    out, _ = O.OracleCFM(sd, arch).sample(ref_mel[None], O.tokens_to_idx([ref_text + gen[0]], vocab), dur, y0=noise[0], steps=steps,
                                          cfg_strength=2.0, sway_sampling_coef=5)
    gmel = out[:, ref_len:, :].permute(0, 2, 1)[0].numpy()
    assert spec.shape == gmel.shape
    mse = float(((spec - gmel) ** 2).mean())
    print(f"\n[infer_batch_process {method}] mel-MSE {mse:.3e}")
    assert mse <= MSE_TOL
    model.engine.close()
