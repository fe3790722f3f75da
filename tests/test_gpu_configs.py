"""GPU: oracle parity at the BASELINE configs beyond the headline HalfCheetah one, and at the
reference's own main.py network.

* Humanoid-v4 (BASELINE configs[3]): O=376, A=17, actor+critic 3x512, W=1.  Policy step, one
  minibatch gradient in f32 and bf16, one full f32 iteration at N=256 T=32 against the oracle,
  and a full-size property iteration (1024 envs per GPU = 8192 / 8, T=128, B=65,536).
* main.py's network (main.py:63-75): O=348, W=5 (in = 1740), actor hidden [256, 256, 128, 128],
  A=17, critic the reference's hard-coded [128, 128] (models/critic.py:14).  Policy step,
  minibatch gradient, full f32 iteration.
* Ant-v4 (BASELINE configs[2]): O=27, A=8, 2x256 with Bernoulli(0.01) terminations (SURVEY.md
  s8(d)): a small-N f32 iteration against the oracle and the N=4096 property iteration on the
  fused bf16 path.
* The HIP forward against tests/golden/reference_mlp.npz, the outputs of the REFERENCE's own
  modules (tests/golden/gen_golden.py), including the 3x512 Humanoid and main.py nets.
"""
import hashlib

import numpy as np
import pytest
import torch

from oracle import ppo_ref as R
from parity_util import (compare_step_grads, load_golden_mlp, make_pair, own_gae,
                         record_oracle_steps, replay_rows, run_iteration_pair, stepwise_parity)

pytestmark = pytest.mark.gpu

HUMANOID = dict(obs=376, act=17, hidden=(512, 512, 512))
MAIN_PY = dict(obs=348, act=17, window=5, hidden=(256, 256, 128, 128), critic_hidden=(128, 128))
ANT = dict(obs=27, act=8, hidden=(256, 256))


def _agent_pair(gpu, seed, n, b, obs, act, hidden, critic_hidden=None, window=1,
                activation="relu", precision="f32"):
    from mujoco_reinforcement_learning_amd.agent import PPOEngineAgent
    from mujoco_reinforcement_learning_amd.runconfig import make_run
    critic_hidden = tuple(critic_hidden or hidden)
    run = make_run(num_envs=n, obs_dim=obs, act_dim=act, window=window, hidden=hidden,
                   critic_hidden=critic_hidden, activation=activation, batch_size=b,
                   precision=precision)
    torch.manual_seed(seed)
    eng = PPOEngineAgent(run, device=gpu, max_rows=max(n, b))
    cfg = R.RefConfig(num_envs=n, obs_dim=obs, act_dim=act, window=window,
                      actor_hidden=tuple(hidden), critic_hidden=critic_hidden,
                      activation=activation, batch_size=b)
    torch.manual_seed(seed)
    ref = R.RefAgent(cfg)
    assert torch.equal(eng.packed_params().cpu(), R.flat_params(ref)), "init differs from oracle"
    return eng, ref


# ------------------------------------------------------------------------- policy step (A1-A4)
@pytest.mark.parametrize("shape,n", [(HUMANOID, 1024), (MAIN_PY, 300)])
def test_policy_step_large_nets(gpu, shape, n):
    obs, act, w = shape["obs"], shape["act"], shape.get("window", 1)
    eng, ref = _agent_pair(gpu, 3, n, n, obs, act, shape["hidden"], shape.get("critic_hidden"), w)
    g = torch.Generator().manual_seed(9)
    state = torch.randn(n, w, obs, generator=g)
    eps = torch.randn(n, act, generator=g)
    sd = state.reshape(n, -1).contiguous().to(gpu)
    action, mean = torch.empty(n, act, device=gpu), torch.empty(n, act, device=gpu)
    logp, value = torch.empty(n, device=gpu), torch.empty(n, device=gpu)
    eng.engine.policy_step(sd, eps=eps.to(gpu), action=action, logp=logp, value=value, mean=mean)
    with torch.no_grad():
        m_ref, s_ref = ref.networks["actor"](state)
        v_ref = ref.networks["critic"](state)[:, 0]
    torch.testing.assert_close(mean.cpu(), m_ref, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(value.cpu(), v_ref, rtol=1e-5, atol=2e-6)
    std = eng.networks["actor"].actor_logstd.detach().exp().cpu()
    assert torch.equal(action.cpu(), eps * std + mean.cpu())  # fl(fl(eps*std)+mean), bit-exact
    lp_ref = torch.distributions.Normal(mean.cpu(), s_ref).log_prob(action.cpu()).sum(dim=1)
    torch.testing.assert_close(logp.cpu(), lp_ref, rtol=1e-6, atol=1e-5)


# --------------------------------------------------------------- minibatch gradient (A11-A13)
def _minibatch_case(gpu, shape, rows_total, b, precision, seed=4, bf16_bar=None):
    obs, act, w = shape["obs"], shape["act"], shape.get("window", 1)
    eng, ref = _agent_pair(gpu, seed, rows_total, b, obs, act, shape["hidden"],
                           shape.get("critic_hidden"), w, precision=precision)
    g = torch.Generator().manual_seed(10)
    states = torch.randn(rows_total, w * obs, generator=g)
    actions = torch.randn(rows_total, act, generator=g) * 0.5
    adv = torch.randn(rows_total, generator=g)
    vt = torch.randn(rows_total, generator=g) * 2
    with torch.no_grad():
        m_ref, s_ref = ref.networks["actor"](states)
        lp = torch.distributions.Normal(m_ref, s_ref).log_prob(actions).sum(1)
    old_logp = lp + torch.randn(rows_total, generator=g) * 0.2  # ratios on both sides of the clip
    rows = torch.randperm(rows_total, generator=g)[:b].to(torch.int32)
    grad = torch.empty(eng.engine.n_params, device=gpu)
    loss = torch.empty(2, device=gpu)
    eng.engine.minibatch_grad(states.to(gpu), actions.to(gpu), old_logp.to(gpu), adv.to(gpu),
                              vt.to(gpu), rows.to(gpu), b, grad, loss, 0.9, 1.1, 1e-4, 1.0 / b,
                              1.0 / (b * act))
    if precision == "bf16":
        R.use_bf16_gemms(ref)
    lc, la, ref_g = _oracle_loss_grads(ref, states, actions, old_logp, adv, vt, rows, b, w, obs,
                                       torch.float32)
    if precision == "bf16":
        # the bar's reference: the same bf16-rounded operands accumulated in f64.  The f32-
        # accumulated emulation differs from it by bf16 rounding flips of intermediates (the
        # engine's MFMA order flips different ones), so the engine is held to the f64 value with
        # a fixed bar, not to the f32 emulation's own spread
        ref.networks.to(torch.float64)
        ref_g = _oracle_loss_grads(ref, states, actions, old_logp, adv, vt, rows, b, w, obs,
                                   torch.float64)[2]
    gd = eng.packed(grad).cpu().double()
    worst, worst_l2, off, bad = 0.0, 0.0, 0, []
    # f32: summation order only.  bf16 vs the f64-accumulated emulation: bf16 rounding flips of
    # intermediates (1 bf16 ulp = 2^-8 relative) through 3 hidden layers of 512
    bar, bar_l2 = (2e-5, 2e-5) if precision == "f32" else (bf16_bar or BF16_GRAD_BAR)
    for name, r_ in ref_g:
        k = r_.numel()
        a = gd[off:off + k]
        scale = float(r_.abs().max()) + 1e-12
        err = float((a - r_).abs().max()) / scale
        l2 = float((a - r_).norm() / (r_.norm() + 1e-20))
        worst, worst_l2 = max(worst, err), max(worst_l2, l2)
        print(f"minibatch grad {precision} {name}: err {err:.3e} of max, rel L2 {l2:.3e}")
        if not (err <= bar and l2 <= bar_l2):
            bad.append((name, err, l2, scale))
        off += k
    print(f"minibatch grad {precision}: worst per-tensor error {worst:.3e} of max (bar {bar}), "
          f"rel L2 {worst_l2:.3e} (bar {bar_l2})")
    assert not bad, bad
    lt = 1e-5 if precision == "f32" else 1e-3
    assert abs(float(loss[1]) - lc) <= lt * (abs(lc) + 1e-2)
    assert abs(float(loss[0]) - la) <= max(lt, 1e-4) * (abs(la) + 1e-2)


# bf16 gradients against the f64-accumulated bf16 emulation: max error per tensor / its max,
# relative L2 per tensor
BF16_GRAD_BAR = (1e-2, 5e-3)


def _oracle_loss_grads(ref, states, actions, old_logp, adv, vt, rows, b, w, obs, dtype):
    """ppo.py:109-135's minibatch loss on the oracle nets in ``dtype`` and its gradient in
    parameters() order: (critic loss, actor loss, [(name, f64 grad)])."""
    idx = rows.long()
    x = states[idx].reshape(b, w, obs).to(dtype)
    _, dist = ref.act(x, return_dist=True)
    new_lp = dist.log_prob(actions[idx].to(dtype)).sum(dim=1)
    v = ref.get_state_value(x)
    lc = torch.nn.functional.huber_loss(v, vt[idx][:, None].to(dtype), reduction="mean")
    ratio = (new_lp - old_logp[idx].to(dtype)).exp()[:, None]
    a_ = adv[idx][:, None].to(dtype)
    la = -torch.min(ratio * a_, torch.clamp(ratio, 0.9, 1.1) * a_).mean() \
        - dist.entropy().mean() * 1e-4
    ref.networks.zero_grad()
    (la + lc).backward()
    grads = [(n, p.grad.double().flatten()) for n, p in ref.networks.named_parameters()]
    return float(lc.detach()), float(la.detach()), grads


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_minibatch_grad_humanoid(gpu, precision):
    _minibatch_case(gpu, HUMANOID, 4096, 2048, precision)


def test_minibatch_grad_main_py_network(gpu):
    _minibatch_case(gpu, MAIN_PY, 1000, 500, "f32")


def test_minibatch_grad_humanoid_bf16_paired_launches(gpu, monkeypatch):
    """At minibatch sizes above 4,096 rows the wide path runs each hidden layer's WGRAD and DGRAD
    as one wide_pair_kernel launch (DGRAD writing dZ to its own buffer): held to the
    f64-accumulated bf16 emulation at the bench's B_local = 8,192, and bitwise equal to the two
    separate launches (PPO_WIDE_PAIR0=1) -- gradient and losses.  The kernels are bitwise
    deterministic, so the bar sits at <= 1.3x the observed value: observed
    1.141e-2 of max on one critic element (four times the rows of the 2,048-row case in every
    weight-gradient column sum, so more bf16 rounding flips of intermediates behind one element)
    and 1.849e-3 relative L2 -> bars 1.45e-2 / 2.4e-3."""
    _minibatch_case(gpu, HUMANOID, 16384, 8192, "bf16", bf16_bar=(1.45e-2, 2.4e-3))
    eng, _ = _agent_pair(gpu, 4, 16384, 8192, HUMANOID["obs"], HUMANOID["act"],
                         HUMANOID["hidden"], None, 1, precision="bf16")
    g = torch.Generator().manual_seed(11)
    n, b, obs, act = 16384, 8192, HUMANOID["obs"], HUMANOID["act"]
    args = [t.to(gpu) for t in (torch.randn(n, obs, generator=g),
                                torch.randn(n, act, generator=g) * 0.5,
                                torch.randn(n, generator=g) - 3, torch.randn(n, generator=g),
                                torch.randn(n, generator=g))]
    rows = torch.randperm(n, generator=g)[:b].to(torch.int32).to(gpu)
    outs = []
    for pair0 in (False, True):
        if pair0:
            monkeypatch.setenv("PPO_WIDE_PAIR0", "1")
        grad, loss = torch.empty(eng.engine.n_params, device=gpu), torch.empty(2, device=gpu)
        eng.engine.minibatch_grad(*args, rows, b, grad, loss, 0.9, 1.1, 1e-4, 1.0 / b,
                                  1.0 / (b * act))
        torch.cuda.synchronize()
        outs.append((grad.clone(), loss.clone()))
    monkeypatch.delenv("PPO_WIDE_PAIR0")
    assert torch.equal(outs[0][0], outs[1][0]), int((outs[0][0] != outs[1][0]).sum())
    assert torch.equal(outs[0][1], outs[1][1])


# ----------------------------------------------------------------- full iteration vs oracle
def _iteration_case(gpu, label, n, t, b, epochs, p_term, strict=False, **shape):
    """Free-running iteration + step-wise parity of each of its E*M optimizer steps.

    Free-running (engine and oracle each on their own trajectory): rollout within 1e-5, GAE of
    the engine's rollout bit-exact, the first step's gradient within 1e-5 of each tensor's max,
    and after all 8 Adam steps every parameter within 2*lr*steps of the oracle with the update
    (post - init) within 1e-3 relative L2 per tensor.  Over 8 steps at 10^6 parameters the
    f32 summation-order noise (MFMA vs MKL) is amplified chaotically by Adam: a near-zero
    gradient component that flips sign moves its parameter by ~2*lr and perturbs every later
    gradient, so the element-wise 1e-5 bar is applied step by step instead:
    Step-wise (stepwise_parity): every step restarted from the oracle's own state lands within
    rtol 1e-5 of the oracle's post-step parameters, except elements whose gradient sign differs
    (counted; only allowed for |g| < 1e-3 of the tensor's max)."""
    algo, agent, ref, env, cfg = make_pair(gpu, n=n, t=t, b=b, epochs=epochs, p_term=p_term,
                                           **shape)
    p0 = R.flat_params(ref).clone()
    steps = record_oracle_steps(ref)
    mem, ref_mem, g_eng, g_ref = run_iteration_pair(algo, agent, ref, env, cfg, seed_train=99)
    adv_own, vt_own = own_gae(mem, cfg)
    assert torch.equal(mem["advantage"].cpu(), adv_own), "GAE on the engine's rollout not bit-exact"
    assert torch.equal(mem["current_state_value_target"].cpu(), vt_own)
    for key in ("current_state", "action", "current_state_value"):
        torch.testing.assert_close(mem[key].cpu(), ref_mem[key], rtol=1e-5, atol=1e-5, msg=key)
    assert torch.equal(mem["terminated"].cpu(), ref_mem["terminated"])
    worst = compare_step_grads(g_eng, g_ref, ref, rel=1e-5, steps=1)
    p_eng, p_ref = agent.packed_params().cpu(), R.flat_params(ref)
    lr = cfg.learning_rate
    assert float((p_eng - p_ref).abs().max()) <= 2 * lr * len(g_ref)
    worst_l2, off = 0.0, 0
    for name, p in ref.networks.named_parameters():
        k = p.numel()
        du_e, du_r = p_eng[off:off + k] - p0[off:off + k], p_ref[off:off + k] - p0[off:off + k]
        worst_l2 = max(worst_l2, float((du_e - du_r).norm() / (du_r.norm() + 1e-20)))
        off += k
    print(f"{label}: first-step grad worst {worst:.3e} of max; free-running update rel L2 "
          f"{worst_l2:.3e}")
    assert worst_l2 <= 1e-3, worst_l2
    rows = replay_rows(99, n, t, b, epochs, cfg.act_dim)
    assert len(rows) == len(steps) == epochs * (n * t // b)
    return stepwise_parity(algo, agent, ref, cfg, ref_mem, steps, rows, label=label, strict=strict)


def test_iteration_humanoid_f32(gpu):
    _iteration_case(gpu, "humanoid 3x512", n=256, t=32, b=2048, epochs=2, p_term=0.02, **HUMANOID)


def test_iteration_humanoid_tanh_f32(gpu):
    """The Humanoid shapes (3x512, O=376, A=17) with tanh: no ReLU kinks, so the step-wise bar
    runs strict -- no float64 arbitration, no kink or oracle-off exemptions; only the counted
    tiny-gradient set (Adam's scale-free step) may leave rtol 1e-5.  Isolates the ReLU case's
    exemptions as kink effects."""
    tot = _iteration_case(gpu, "humanoid 3x512 tanh", n=256, t=32, b=2048, epochs=2, p_term=0.02,
                          strict=True, activation="tanh", **HUMANOID)
    assert tot.get("f64_arbitrated", 0) == 0 and tot.get("engine_kink_elements", 0) == 0


def test_iteration_main_py_network_f32(gpu):
    _iteration_case(gpu, "main.py net", n=64, t=32, b=512, epochs=2, p_term=0.02, **MAIN_PY)


def test_iteration_ant_terminations_f32(gpu):
    _iteration_case(gpu, "ant 2x256", n=128, t=32, b=1024, epochs=2, p_term=0.01, **ANT)


# --------------------------------------------------- full-size property iterations (no oracle)
@pytest.mark.parametrize("label,shape,n,precision", [
    ("humanoid 1024 envs/GPU", HUMANOID, 1024, "bf16"),
    ("ant 4096 envs", ANT, 4096, "bf16")])
def test_full_size_iteration_properties(gpu, label, shape, n, precision):
    """BASELINE shapes at full size (Humanoid: 8192 envs over 8 GPUs = 1024 per GPU; Ant: 4096
    envs with Bernoulli(0.01) terminations), T=128, B=65,536, one epoch: the GAE of the engine's
    own rollout is bit-exact against the oracle's recurrence, every output is finite, the
    parameters move, and a second run from the same seeds is bit-identical."""
    outs = []
    for _ in range(2):
        algo, agent, ref, env, cfg = make_pair(gpu, n=n, t=128, b=65536, epochs=1, p_term=0.01,
                                               rng="philox", seed=2, precision=precision, **shape)
        p0 = agent.packed_params().clone()
        algo.iterate(verbose=False)
        torch.cuda.synchronize()
        mem = algo.buffer
        adv_own, vt_own = own_gae(mem, cfg)
        assert torch.equal(mem["advantage"].cpu(), adv_own), label
        assert torch.equal(mem["current_state_value_target"].cpu(), vt_own), label
        assert bool(mem["terminated"].any()), "Bernoulli(0.01) terminations expected"
        p1 = agent.packed_params()
        assert bool(torch.isfinite(p1).all()) and not torch.equal(p0, p1)
        assert all(np.isfinite(x) for x in algo.last_losses)
        outs.append(p1.cpu())
    assert torch.equal(outs[0], outs[1]), f"{label}: not bit-reproducible"


# --------------------------------------------- HIP forward against the reference's own outputs
def _golden_cases():
    return sorted({k.split("/")[0] for k in load_golden_mlp()})


@pytest.mark.parametrize("name", _golden_cases())
def test_hip_forward_matches_reference_golden(gpu, name):
    """tests/golden/reference_mlp.npz holds the reference modules' (models/linear/actor.py,
    network_block_creator.py) forward outputs on a fixed input, with their parameters (nets up to
    2x256) or the sha256 of every parameter (the 3x512 Humanoid and main.py nets).  With the
    stored parameters loaded, the HIP forward must reproduce the reference's mean / std / value
    within f32 summation order (rtol 1e-5).  Without them the engine's seeded init is used: it
    replays the reference's RNG order (pinned bit-exact by tests/test_oracle.py in the container
    that generated the fixture), but the orthogonal init goes through the host's LAPACK QR, whose
    last bits may differ on the GPU box's CPU -- far below the 1e-5 forward bar."""
    from mujoco_reinforcement_learning_amd.agent import PPOEngineAgent
    from mujoco_reinforcement_learning_amd.runconfig import make_run
    z = load_golden_mlp()
    seed, obs, window, act, n_a, n_c, *widths = (int(v) for v in z[f"{name}/meta"])
    hidden, critic_hidden = widths[:n_a], widths[n_a:n_a + n_c]
    activation = str(z[f"{name}/activation"])
    x = torch.from_numpy(z[f"{name}/x"])
    run = make_run(num_envs=len(x), obs_dim=obs, act_dim=act, window=window, hidden=hidden,
                   critic_hidden=critic_hidden, activation=activation, batch_size=len(x))
    torch.manual_seed(seed)
    agent = PPOEngineAgent(run, device=gpu)
    sd = agent.networks.state_dict()
    if all(f"{name}/{k}" in z for k in sd):
        agent.networks.load_state_dict({k: torch.from_numpy(z[f"{name}/{k}"]) for k in sd})
        for k, v in agent.networks.state_dict().items():
            digest = hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
            assert digest == str(z[f"{name}/sha256/{k}"]), k
    st = x.reshape(len(x), -1).contiguous().to(gpu)
    mean = torch.empty(len(x), act, device=gpu)
    value = torch.empty(len(x), device=gpu)
    agent.engine.policy_step(st, mean=mean, value=value)
    torch.testing.assert_close(mean.cpu(), torch.from_numpy(z[f"{name}/mean"]), rtol=1e-5,
                               atol=1e-6)
    torch.testing.assert_close(value.cpu(), torch.from_numpy(z[f"{name}/value"])[:, 0], rtol=1e-5,
                               atol=1e-6)
    std = agent.networks["actor"].actor_logstd.detach().exp().cpu()
    assert torch.equal(std[None].expand(len(x), -1), torch.from_numpy(z[f"{name}/std"]))


# --------------------------------------------- bf16 policy step on the wide path (Humanoid shapes)
def test_policy_step_humanoid_bf16(gpu):
    """The rollout step on the wide bf16-resident path (csrc/wide_engine.hip) against the bf16
    emulation oracle (operands rounded to bf16, f32 accumulation): mean / value within 1e-2 of
    their scale (bf16 rounding of 3 hidden layers' outputs, different summation order), the
    action exactly fl(fl(eps*std)+mean) of the engine's own mean, log-prob from that action."""
    shape, n = HUMANOID, 1024
    obs, act = shape["obs"], shape["act"]
    eng, ref = _agent_pair(gpu, 3, n, n, obs, act, shape["hidden"], precision="bf16")
    R.use_bf16_gemms(ref)
    g = torch.Generator().manual_seed(9)
    state = torch.randn(n, 1, obs, generator=g)
    eps = torch.randn(n, act, generator=g)
    sd = state.reshape(n, -1).contiguous().to(gpu)
    action, mean = torch.empty(n, act, device=gpu), torch.empty(n, act, device=gpu)
    logp, value = torch.empty(n, device=gpu), torch.empty(n, device=gpu)
    eng.engine.policy_step(sd, eps=eps.to(gpu), action=action, logp=logp, value=value, mean=mean)
    with torch.no_grad():
        m_ref, s_ref = ref.networks["actor"](state)
        v_ref = ref.networks["critic"](state)[:, 0]
    for got, want in ((mean.cpu(), m_ref), (value.cpu(), v_ref)):
        err = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12)
        l2 = float((got - want).norm() / (want.norm() + 1e-20))
        print(f"bf16 policy step: max err {err:.3e} of scale, rel L2 {l2:.3e}")
        assert err <= 1e-2 and l2 <= 5e-3
    std = eng.networks["actor"].actor_logstd.detach().exp().cpu()
    assert torch.equal(action.cpu(), eps * std + mean.cpu())
    lp_ref = torch.distributions.Normal(mean.cpu(), std).log_prob(action.cpu()).sum(dim=1)
    torch.testing.assert_close(logp.cpu(), lp_ref, rtol=1e-6, atol=1e-5)
