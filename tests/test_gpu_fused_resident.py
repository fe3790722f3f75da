"""The fused update kernel's resident schedule (PPO_FUSED_SCHED=3, fused_body SCHED bit 1): the
first k-steps of the W1^T stream held in LDS for the whole launch, d2 written in place of a2, the
dgrad product transposed and D1 fed to dW0 from registers.  It moves data between LDS, registers
and phases only: every result is bitwise that of schedules 0 and 1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RESIDENT = 3
HYPER = dict(one_minus_beta1=0.1, beta2=0.999, one_minus_beta2=0.001, eps=1e-8)


def _agent(gpu, seed, **kw):
    from mujoco_reinforcement_learning_amd.agent import PPOEngineAgent
    from mujoco_reinforcement_learning_amd.runconfig import make_run
    run = make_run(hidden=(256, 256), precision="bf16", **kw)
    torch.manual_seed(seed)
    return PPOEngineAgent(run, device=gpu)


def _data(gpu, n, t, b, obs, act, seed, nrows=2):
    g = torch.Generator().manual_seed(seed)
    d = dict(states=torch.randn(t + 1, n, obs, generator=g).to(gpu),
             actions=torch.randn(t, n, act, generator=g).to(gpu),
             old_lp=(torch.randn(t, n, generator=g) - 5).to(gpu),
             adv=torch.randn(t, n, generator=g).to(gpu),
             vt=torch.randn(t, n, generator=g).to(gpu))
    # distinct rows where the storage has b of them, else drawn with repeats
    rows = [(torch.randperm(n * t, generator=g)[:b] if b <= n * t
             else torch.randint(0, n * t, (b,), generator=g)).to(torch.int32).to(gpu)
            for _ in range(nrows)]
    return d, rows, g


def _two_steps(eng, gpu, monkeypatch, scheds, n, t, b, obs=17, act=6, count=None, seed=9):
    """Two chained update_step_staged calls (and, with `count`, a minibatch_grad_staged with that
    device row count on the updated weights) under each schedule, from the same start."""
    e = eng.engine
    assert e.fused
    d, rows, g = _data(gpu, n, t, b, obs, act, seed)
    args = (0.9, 1.1, 1e-4, 1.0 / b, 1.0 / (b * act))
    p0 = eng.flat_params.clone()
    m0 = torch.rand(e.n_params, generator=g).to(gpu) * 1e-3
    v0 = torch.rand(e.n_params, generator=g).to(gpu) * 1e-6
    e.stage_records(d["states"], d["actions"], d["old_lp"], d["adv"], d["vt"])
    cnt = torch.tensor([count], dtype=torch.int32, device=gpu) if count is not None else None
    outs = {}
    for s in scheds:
        monkeypatch.setenv("PPO_FUSED_SCHED", str(s))
        eng.flat_params.copy_(p0)
        m, v = m0.clone(), v0.clone()
        e.pack_weights()
        res = []
        for k in range(2):
            grad, loss = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
            e.update_step_staged(rows[k], b, grad, loss, m, v, *args, neg_step_actor=-1e-3,
                                 neg_step_critic=-2e-3, bc2_sqrt=0.3,
                                 next_rows=rows[1] if k == 0 else None,
                                 weights_current=k > 0, rows_gathered=k > 0, **HYPER)
            res += [grad.clone(), loss.clone()]
        if cnt is not None:
            gc, lc = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
            e.minibatch_grad_staged(rows[1], b, gc, lc, *args, count=cnt, weights_current=True)
            res += [gc, lc]
        torch.cuda.synchronize()
        outs[s] = res + [eng.flat_params.clone(), m, v]
    return outs


def _assert_bitwise(outs, base, others):
    assert bool(torch.isfinite(outs[base][0]).all()) and float(outs[base][0].abs().max()) > 0
    for s in others:
        for i, (x, y) in enumerate(zip(outs[base], outs[s])):
            assert torch.equal(x, y), (s, i, int((x != y).sum()))


@pytest.mark.parametrize("n,t,b", [(64, 2, 64), (64, 2, 100), (512, 16, 8256)])
def test_resident_schedule_bitwise(gpu, monkeypatch, n, t, b):
    """Against schedules 0 and 1: one chunk in one workgroup (b = 64), a masked partial chunk
    (b = 100), and 129 chunks over 128 workgroups (b = 8256: workgroups with two chunks, with one,
    and a masked last chunk)."""
    eng = _agent(gpu, 15, num_envs=n, batch_size=b)
    outs = _two_steps(eng, gpu, monkeypatch, (0, 1, RESIDENT), n, t, b)
    _assert_bitwise(outs, 0, (1, RESIDENT))


@pytest.mark.parametrize("obs,act,use_bias", [(3, 1, True), (27, 8, True), (32, 2, False)])
def test_resident_schedule_other_widths(gpu, monkeypatch, obs, act, use_bias):
    """Other input and head widths (the head instantiations NH = 2 and 8; input widths 3, 27 and
    the full 32), once without biases, each with a device row count below b."""
    n, t, b = 128, 4, 300
    eng = _agent(gpu, 16, num_envs=n, batch_size=b, obs_dim=obs, act_dim=act, use_bias=use_bias)
    outs = _two_steps(eng, gpu, monkeypatch, (0, 1, RESIDENT), n, t, b, obs=obs, act=act,
                      count=b - 77, seed=10)
    _assert_bitwise(outs, 0, (1, RESIDENT))


@pytest.mark.parametrize("activation", ["tanh", "elu"])
def test_resident_schedule_leaves_tanh_elu_alone(gpu, monkeypatch, activation):
    """tanh / ELU have one schedule: with the resident one selected they give schedule 0's bits."""
    n, t, b = 128, 4, 300
    eng = _agent(gpu, 17, num_envs=n, batch_size=b, activation=activation)
    outs = _two_steps(eng, gpu, monkeypatch, (0, RESIDENT), n, t, b, seed=11)
    _assert_bitwise(outs, 0, (RESIDENT,))


def test_resident_weights_follow_the_tail(gpu, monkeypatch):
    """The resident copy is per launch: after two steps on the images the tail rewrote
    (weights_current=True), the next gradient equals the one computed after pack_weights()
    rebuilt every image from the parameters."""
    n, t, b = 128, 4, 300
    monkeypatch.setenv("PPO_FUSED_SCHED", str(RESIDENT))
    eng = _agent(gpu, 18, num_envs=n, batch_size=b)
    e = eng.engine
    assert e.fused
    d, rows, g = _data(gpu, n, t, b, 17, 6, 12, nrows=3)
    args = (0.9, 1.1, 1e-4, 1.0 / b, 1.0 / (b * 6))
    m = torch.rand(e.n_params, generator=g).to(gpu) * 1e-3
    v = torch.rand(e.n_params, generator=g).to(gpu) * 1e-6
    e.stage_records(d["states"], d["actions"], d["old_lp"], d["adv"], d["vt"])
    e.pack_weights()
    p0 = eng.flat_params.clone()
    grads = []
    for k in range(3):  # step 0 on the packed images, steps 1 and 2 on the tail's
        grad, loss = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
        if k == 2:
            p2, m2, v2 = eng.flat_params.clone(), m.clone(), v.clone()
        e.update_step_staged(rows[k], b, grad, loss, m, v, *args, neg_step_actor=-1e-2,
                             neg_step_critic=-2e-2, bc2_sqrt=0.3, weights_current=k > 0, **HYPER)
        grads.append((grad.clone(), loss.clone()))
    assert not torch.equal(p2, p0)
    eng.flat_params.copy_(p2)
    e.pack_weights()
    gf, lf = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
    e.minibatch_grad_staged(rows[2], b, gf, lf, *args, weights_current=True)
    torch.cuda.synchronize()
    assert torch.equal(grads[2][0], gf), int((grads[2][0] != gf).sum())
    assert torch.equal(grads[2][1], lf)
    # and the weights did move the gradient: the same rows on the first images differ
    eng.flat_params.copy_(p0)
    e.pack_weights()
    g0 = torch.empty(e.n_params, device=gpu)
    e.minibatch_grad_staged(rows[2], b, g0, lf, *args, weights_current=True)
    torch.cuda.synchronize()
    assert not torch.equal(g0, gf)
