"""Per-phase cycles of one step of the persistent rollout's loop body (ppo_rollout_synthetic, ReLU
2x256, O=17, A=6, N=4096, T=128) from the stamped diagnostic instantiation: wave 0's s_memtime
deltas per phase, the mean over the T steps, averaged over workgroups -- the same format as
tools/policy_phases.py prints for the per-step kernel."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PHASES = ["step t+1's stream loads issued (base_obs, noise, reward, termination)",
          "per-(row, slice) f64 mean / std, standardised state -> X image + state out, barrier",
          "L0 MFMA + act -> A1, barrier", "L1 MFMA pass (W1 in registers)",
          "act -> A2 image, barrier", "head MFMAs + wave-pair exchange (barrier inside)",
          "tanh, sample, logp, action / logp stores, action image, barrier",
          "env: reward / termination out, next observation"]


def main():
    from mujoco_reinforcement_learning_amd.agent import PPOEngineAgent
    from mujoco_reinforcement_learning_amd.environments import make_synthetic_streams
    from mujoco_reinforcement_learning_amd.runconfig import make_run
    dev = torch.device("cuda", 0)
    n, t, o, a = 4096, 128, 17, 6
    run = make_run(num_envs=n, horizon=t, hidden=(256, 256), rng="philox", precision="bf16")
    torch.manual_seed(0)
    agent = PPOEngineAgent(run, device=dev)
    e = agent.engine
    e.pack_weights()
    st = make_synthetic_streams(n, t, o, seed=1, device="cuda")
    win = st["base_obs"][0].double().view(n, o, 1).contiguous()
    states = torch.empty(t + 1, n, o, device=dev)
    noise = torch.randn(t, n, a, device=dev)
    act, lp = torch.empty(t, n, a, device=dev), torch.empty(t, n, device=dev)
    rew = torch.empty(t, n, device=dev, dtype=torch.float64)
    term = torch.empty(t, n, device=dev, dtype=torch.bool)
    for rep in range(3):
        e.phase_stamps(True)
        e.rollout_synthetic(st["base_obs"], st["base_reward"], st["base_terminated"], win, True,
                            states, noise, act, lp, rew, term)
        # the step kernel's layout: 11 slots per workgroup (phase_stamps views them as 13)
        s = e.phase_stamps(False).flatten()[:2 * 128 * 11].view(2, 128, 11).double()
    rows = s[0, :n // 32]
    tot = rows[:, 9].mean()
    print(f"rollout loop body: {tot:.0f} cycles per step and workgroup (wave 0, mean over {t} "
          f"steps and {n // 32} workgroups)")
    for k, ph in enumerate(PHASES):
        print(f"   {rows[:, k].mean():8.0f}  {100 * rows[:, k].mean() / tot:5.1f}%  {ph}")


if __name__ == "__main__":
    main()
