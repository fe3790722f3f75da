"""The fused update kernel's packed constants image (one per net: the kernel's per-launch LDS
constants in their LDS layout, copied by its prologue instead of being rebuilt from the f32
parameters) and the one-launch row indices of the update loop.

Hidden (256, 256), precision bf16, 64 envs x 9 steps staged, minibatches of 64 rows (one chunk,
one workgroup per net) and 320 rows (5 workgroups); every comparison is torch.equal, except the
three values derived from log-std, which are compared bitwise between the writers and must be
equal or adjacent f32 values against the same f32 operations in torch.

The image, restated here from the kernel's layout table (H = 256; byte offsets):
    0       bf16 head image [16][H + 8]: row a < heads = bf16(W_h[a]), 8 zero pad; rows >= heads zero
    8448    f32 b0[H], b1[H] (zero without biases)
    10496   f32 [80]: b_h[16], log-std[16], log(std)[16], 1/var[16], 1/(2 var)[16]; a head without
            parameters holds 0, 0, 0, 1, 0.5
    10816   bf16 W0 image [H][32]: 64-B rows, 16-B chunk c of row f at 16 (c ^ ((f >> 2) & 3)),
            columns >= obs zero
    27200   bf16 W_h^T [H][16]: (f, a) = bf16(W_h[a][f]), columns >= heads zero
    35392   end
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ENVS, T_STEPS, H = 64, 9, 256
ARGS = (0.9, 1.1, 1e-4)
HYPER = dict(one_minus_beta1=0.1, beta2=0.999, one_minus_beta2=0.001, eps=1e-8)
SC = [(-1e-3, -2e-3, 0.3), (-1.5e-3, -2.5e-3, 0.4)]
OFF_BIAS, OFF_HS, OFF_W0, OFF_WHT, IMG_BYTES = 8448, 10496, 10816, 27200, 35392


def _setup(gpu, seed, b, act_dim, obs_dim, activation, use_bias=True):
    from mujoco_reinforcement_learning_amd.agent import PPOEngineAgent
    from mujoco_reinforcement_learning_amd.runconfig import make_run
    run = make_run(num_envs=N_ENVS, hidden=(H, H), batch_size=b, precision="bf16",
                   act_dim=act_dim, obs_dim=obs_dim, activation=activation, use_bias=use_bias)
    torch.manual_seed(seed)
    eng = PPOEngineAgent(run, device=gpu)
    e = eng.engine
    assert e.fused
    g = torch.Generator().manual_seed(seed + 100)
    n, t = N_ENVS, T_STEPS
    # every parameter off its initial value (log-std and the biases start at zero)
    eng.flat_params.add_(0.05 * torch.randn(e.n_params, generator=g).to(gpu))
    ls0 = e.param_offsets()[0]
    eng.flat_params[ls0:ls0 + act_dim] = (-0.5 + 0.3 * torch.randn(act_dim, generator=g)).to(gpu)
    states = torch.randn(t + 1, n, obs_dim, generator=g).to(gpu)
    actions = torch.randn(t, n, act_dim, generator=g).to(gpu)
    old_lp = torch.randn(t, n, generator=g).to(gpu) - 5
    adv = torch.randn(t, n, generator=g).to(gpu)
    vt = torch.randn(t, n, generator=g).to(gpu)
    rows = [torch.randperm(n * t, generator=g)[:b].to(torch.int32).to(gpu) for _ in range(3)]
    m0 = torch.rand(e.n_params, generator=g).to(gpu) * 1e-3
    v0 = torch.rand(e.n_params, generator=g).to(gpu) * 1e-6
    e.stage_records(states, actions, old_lp, adv, vt)
    args = ARGS + (1.0 / b, 1.0 / (b * act_dim))
    return eng, e, rows, args, eng.flat_params.clone(), m0, v0


def _tensors(e, flat, net, act_dim, obs_dim, use_bias):
    """(log-std, W0, b0, W1, b1, W_h, b_h) of net 0 / 1 from the flat parameters (None: absent)."""
    offs = e.param_offsets()
    n_actor = 1 + (6 if use_bias else 3)
    offs = offs[:n_actor] if net == 0 else offs[n_actor:]
    bias = use_bias if net == 0 else True
    heads = act_dim if net == 0 else 1
    it = iter(offs)

    def take(*shape):
        o = next(it)
        n = 1
        for s in shape:
            n *= s
        return flat[o:o + n].view(*shape)
    ls = take(act_dim) if net == 0 else None
    w0 = take(H, obs_dim)
    b0 = take(H) if bias else None
    w1 = take(H, H)
    b1 = take(H) if bias else None
    wh = take(heads, H)
    bh = take(heads) if bias else None
    return ls, w0, b0, w1, b1, wh, bh


def _bf16_bytes(x):
    return x.to(torch.bfloat16).contiguous().view(torch.uint8).flatten()


def _f32_bytes(x):
    return x.to(torch.float32).contiguous().view(torch.uint8).flatten()


def _expected(e, flat, net, act_dim, obs_dim, use_bias):
    """The image rebuilt in torch (on the parameters' device), as uint8 on the host, and the byte
    ranges of the three fields derived from log-std."""
    ls, w0, b0, _, b1, wh, bh = _tensors(e, flat, net, act_dim, obs_dim, use_bias)
    dev = flat.device
    heads = wh.shape[0]
    head = torch.zeros(16, H + 8, device=dev)
    head[:heads, :H] = wh
    bias = torch.zeros(2, H, device=dev)
    if b0 is not None:
        bias[0], bias[1] = b0, b1
    hs = torch.zeros(5, 16, device=dev)
    hs[3], hs[4] = 1.0, 0.5
    if bh is not None:
        hs[0, :heads] = bh
    if ls is not None:
        sd = torch.exp(ls)
        var = sd * sd
        hs[1, :heads] = ls
        hs[2, :heads] = torch.log(sd)
        hs[3, :heads] = 1.0 / var
        hs[4, :heads] = 1.0 / (2.0 * var)
    w0p = torch.zeros(H, 32, device=dev)
    w0p[:, :obs_dim] = w0
    f = torch.arange(H, device=dev).view(H, 1)
    c = torch.arange(4, device=dev).view(1, 4)
    w0img = torch.zeros(H, 4, 8, device=dev)
    w0img[f.expand(H, 4), (c ^ ((f >> 2) & 3))] = w0p.view(H, 4, 8)
    wht = torch.zeros(H, 16, device=dev)
    wht[:, :heads] = wh.t()
    img = torch.cat([_bf16_bytes(head), _f32_bytes(bias), _f32_bytes(hs), _bf16_bytes(w0img),
                     _bf16_bytes(wht)]).cpu()
    assert img.numel() == IMG_BYTES
    return img, (OFF_HS + 4 * 32, OFF_HS + 4 * 80)


def _adjacent_or_equal(a, b):
    return bool(((a == b) | (torch.nextafter(a, b) == b)).all())


def _check_image(e, flat, net, act_dim, obs_dim, use_bias):
    got = e.fused_constants(net)
    want, (d0, d1) = _expected(e, flat, net, act_dim, obs_dim, use_bias)
    assert got.numel() == IMG_BYTES
    assert torch.equal(got[:d0], want[:d0]), (net, int((got[:d0] != want[:d0]).sum()))
    assert torch.equal(got[d1:], want[d1:]), (net, int((got[d1:] != want[d1:]).sum()))
    gd, wd = got[d0:d1].view(torch.float32), want[d0:d1].view(torch.float32)
    assert _adjacent_or_equal(gd, wd), (net, gd, wd)
    return got


SHAPES = [
    # b, act_dim, obs_dim, activation, use_bias
    (64, 1, 11, "relu", True),
    (320, 3, 17, "tanh", True),
    (320, 6, 32, "elu", True),
    (320, 8, 17, "relu", True),
    (64, 8, 32, "relu", False),
    (320, 3, 11, "tanh", False),
    (64, 6, 17, "elu", False),
    (320, 1, 32, "tanh", False),
]


@pytest.mark.parametrize("b,act_dim,obs_dim,activation,use_bias", SHAPES)
def test_image_bytes_after_pack(gpu, b, act_dim, obs_dim, activation, use_bias):
    """After pack_weights() every field of both nets' images is the torch reconstruction from
    flat_params: bf16 by round-to-nearest-even, the W0 swizzle and the head transposition by the
    formulas above, the pads at their fixed values."""
    eng, e, *_ = _setup(gpu, 31, b, act_dim, obs_dim, activation, use_bias)
    e.pack_weights()
    for net in (0, 1):
        _check_image(e, eng.flat_params, net, act_dim, obs_dim, use_bias)
    # a second pack after a change of every parameter overwrites every parameter's bytes
    eng.flat_params.mul_(-1.5)
    e.pack_weights()
    for net in (0, 1):
        _check_image(e, eng.flat_params, net, act_dim, obs_dim, use_bias)


def _images(e):
    return [e.fused_constants(0), e.fused_constants(1)]


def _assert_fresh(eng, e, what, act_dim, obs_dim, use_bias):
    """The images a writer left are byte-equal to the ones pack_weights() then builds from the
    resulting parameters (and those match torch)."""
    left = _images(e)
    e.pack_weights()
    fresh = _images(e)
    for net in (0, 1):
        assert torch.equal(left[net], fresh[net]), (what, net, int((left[net] != fresh[net]).sum()))
        _check_image(e, eng.flat_params, net, act_dim, obs_dim, use_bias)
    return fresh


@pytest.mark.parametrize("b,act_dim,obs_dim,activation,use_bias", SHAPES)
def test_every_writer_agrees(gpu, b, act_dim, obs_dim, activation, use_bias):
    """The step tail (device Adam scalars), adam_pack and the non-reducing tail each leave the
    image that pack_weights() builds from the parameters they produced."""
    eng, e, rows, args, p0, m0, v0 = _setup(gpu, 32, b, act_dim, obs_dim, activation, use_bias)
    shape = (act_dim, obs_dim, use_bias)
    p_start = eng.flat_params.clone()

    # the tail of ppo_update_step_staged, two chained steps
    m, v = m0.clone(), v0.clone()
    e.pack_weights()
    start = _images(e)
    for k in range(2):
        grad, loss = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
        e.update_step_staged(rows[k], b, grad, loss, m, v, *args,
                             next_rows=rows[1] if k == 0 else None, weights_current=k > 0,
                             rows_gathered=k > 0, sched=torch.tensor(SC[k], device=gpu), **HYPER)
    tail = _assert_fresh(eng, e, "step tail", *shape)
    p_tail = eng.flat_params.clone()
    assert not torch.equal(p_tail, p_start)
    assert not torch.equal(tail[0], start[0]) and not torch.equal(tail[1], start[1])

    # the same two steps as minibatch_grad_staged + adam_pack
    eng.flat_params.copy_(p_start)
    m, v = m0.clone(), v0.clone()
    e.pack_weights()
    for k in range(2):
        grad, loss = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
        e.minibatch_grad_staged(rows[k], b, grad, loss, *args, weights_current=k > 0)
        s = dict(zip(("neg_step_actor", "neg_step_critic", "bc2_sqrt"), SC[k]), **HYPER)
        e.adam_pack(grad, m, v, None, **s)
    sep = _assert_fresh(eng, e, "adam_pack", *shape)
    assert torch.equal(eng.flat_params, p_tail)
    for net in (0, 1):
        assert torch.equal(sep[net], tail[net])

    # then the non-reducing tail: adam_pack(next_rows=...)
    grad, loss = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
    e.minibatch_grad_staged(rows[2], b, grad, loss, *args, weights_current=True)
    s = dict(zip(("neg_step_actor", "neg_step_critic", "bc2_sqrt"), SC[0]), **HYPER)
    e.adam_pack(grad, m, v, None, next_rows=rows[0], **s)
    last = _assert_fresh(eng, e, "non-reducing tail", *shape)
    assert not torch.equal(last[0], sep[0]) and not torch.equal(last[1], sep[1])


@pytest.mark.parametrize("b,act_dim,obs_dim,activation,use_bias", [(320, 3, 11, "tanh", True),
                                                                   (64, 8, 32, "relu", False)])
def test_next_gradient_on_the_tail_images(gpu, b, act_dim, obs_dim, activation, use_bias):
    """The next gradient and losses on the images the tail left (weights_current=True) equal
    those after a fresh pack_weights()."""
    eng, e, rows, args, p0, m0, v0 = _setup(gpu, 33, b, act_dim, obs_dim, activation, use_bias)
    m, v = m0.clone(), v0.clone()
    e.pack_weights()
    for k in range(2):
        grad, loss = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
        s = dict(zip(("neg_step_actor", "neg_step_critic", "bc2_sqrt"), SC[k]), **HYPER)
        e.update_step_staged(rows[k], b, grad, loss, m, v, *args,
                             next_rows=rows[1] if k == 0 else None, weights_current=k > 0,
                             rows_gathered=k > 0, **s)
    g1, l1 = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
    e.minibatch_grad_staged(rows[2], b, g1, l1, *args, weights_current=True)
    e.pack_weights()
    g2, l2 = torch.empty(e.n_params, device=gpu), torch.empty(2, device=gpu)
    e.minibatch_grad_staged(rows[2], b, g2, l2, *args, weights_current=True)
    torch.cuda.synchronize()
    assert not torch.equal(eng.flat_params, p0)
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    assert torch.equal(g1, g2), int((g1 != g2).sum())
    assert torch.equal(l1, l2)


@pytest.mark.parametrize("n,t", [(40, 9), (512, 17), (4096, 128)])
@pytest.mark.parametrize("n_epochs", [1, 10])
@pytest.mark.parametrize("epoch0", [0, 37])
def test_feistel_rows_epochs_equals_single_calls(gpu, n, t, n_epochs, epoch0):
    """feistel_rows_epochs over E epochs writes what E feistel_rows calls write: the whole
    permutation and slices with start > 0, into a contiguous buffer and into a column slice of a
    wider one (row stride > b)."""
    from mujoco_reinforcement_learning_amd import engine as E
    total = n * t
    for start, b in ((0, total), (total // 3, total // 2), (total - 5, 5)):
        wide = torch.full((n_epochs, b + 7), -1, dtype=torch.int32, device=gpu)
        many = torch.empty(n_epochs, b, dtype=torch.int32, device=gpu)
        E.feistel_rows_epochs(123, epoch0, start, b, n, t, many)
        E.feistel_rows_epochs(123, epoch0, start, b, n, t, wide[:, :b])
        one = torch.empty(n_epochs, b, dtype=torch.int32, device=gpu)
        for y in range(n_epochs):
            E.feistel_rows(123, epoch0 + y, start, b, n, t, one[y])
        assert torch.equal(many, one), (start, b)
        assert torch.equal(wide[:, :b], one) and bool((wide[:, b:] == -1).all())
        if start == 0:
            assert torch.equal(many.sort(dim=1).values[0].long(), torch.arange(total, device=gpu))
