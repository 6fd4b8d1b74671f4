"""DiscreteCRR on the C3 shape (record, not a gate): 84x84x4 uint8 observations, 6 actions, "exp" mode, lagged networks, at
B = 512 and at B = 32 (the batch size of examples/offline/atari_crr.py) -- beside the DiscreteBCQ engine on the same inputs
and the same CRR update in eager PyTorch on the same GPU, all in one process.

    python bench_crr.py [--steps K] [--warmup W] [--out profiles/crr_bench.json]

One CRR "update" = the live trunk and both heads on s, the lagged trunk and both lagged heads on s' (inside the update: CRR
has no preprocessing pass on the device), the target, the loss, the backward pass through both heads into the shared trunk and
Adam.  DiscreteBCQ does its second network pass in preprocessing, so the comparison is CRR's update against BCQ's
target_q + update; BCQ's update alone and its target pass alone are timed as well, and both sums are reported.  The eager
baseline is the CRR update written out below on the stand-in modules of tests/standin_crr.py moved to the device, with
torch.optim.Adam.  All are timed in alternation, each call on its own with a device synchronisation, after a clock warm-up;
the figure is the median of the timed calls.  No ratio is fixed in advance; one condition is checked: the engine must not be
slower than the eager update.

Class level, a separate line: HipDiscreteCRR.update() over the stand-in classes and a host replay buffer, once with the
stand-in's placeholder `_preprocess_batch` and once with the discounted episodic returns that the reference's base
implementation computes on the host (restated here on oracle/oracle.py's episodic-return routine; the update never reads
them).  The difference of the two is the host cost of keeping that preprocessing.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

C, H, W, N_ACT = 4, 84, 84, 6
GAMMA, LR, FREQ = 0.99, 1e-4, 8000
MODE, BETA, RATIO_UPPER_BOUND, MIN_Q_WEIGHT = "exp", 1.0, 20.0, 10.0
TAU, THETA = 0.3, 1e-2                                  # the BCQ engine's own two scalars


def _stats(times: list[float]) -> dict:
    med = statistics.median(times)
    q = statistics.quantiles(times, n=4)
    return {"updates_per_s_median": 1.0 / med, "updates_per_s_min": 1.0 / max(times), "updates_per_s_max": 1.0 / min(times),
            "ms_per_update_median": med * 1e3, "ms_per_update_q1": q[0] * 1e3, "ms_per_update_q3": q[2] * 1e3}


def _eager():
    """The reference's update restated on the stand-in modules (discrete_crr.py:125-167, both broadcasts kept) -> a callable."""
    import copy

    import torch.nn.functional as F
    from torch.distributions import Categorical

    from tests import standin_crr as SC

    torch.manual_seed(0)
    trunk = SC.DQNetFeaturesOnly(C, H, W)
    actor = SC.DiscreteActor(preprocess_net=trunk, action_shape=N_ACT, hidden_sizes=[512], softmax_output=False).cuda()
    critic = SC.DiscreteCritic(preprocess_net=trunk, hidden_sizes=[512], last_size=N_ACT).cuda()
    actor_old, critic_old = copy.deepcopy(actor), copy.deepcopy(critic)
    opt = torch.optim.Adam(torch.nn.ModuleList([actor, critic]).parameters(), lr=LR)

    def one(obs, obs_next, act, rew, done):
        q_t = critic(obs)
        qa_t = q_t.gather(1, act.unsqueeze(1))
        with torch.no_grad():
            target_a_t, _ = actor_old(obs_next)
            q_t_target = critic_old(obs_next)
            expected = (q_t_target * Categorical(logits=target_a_t).probs).sum(-1, keepdim=True)
            expected[done > 0] = 0.0
            target = rew.unsqueeze(1) + GAMMA * expected
        critic_loss = 0.5 * F.mse_loss(qa_t, target)
        logits, _ = actor(obs)
        dist = Categorical(logits=logits)
        advantage = qa_t - (q_t * dist.probs).sum(-1, keepdim=True)
        coef = (advantage / BETA).exp().clamp(0, RATIO_UPPER_BOUND)
        actor_loss = (-dist.log_prob(act) * coef).mean()
        cql_loss = (q_t.logsumexp(1) - qa_t).mean()
        loss = actor_loss + critic_loss + MIN_Q_WEIGHT * cql_loss
        opt.zero_grad()
        loss.backward()
        opt.step()
        return torch.stack([loss.detach(), actor_loss.detach(), critic_loss.detach(), cql_loss.detach()]).tolist()

    return one


def run_batch(batch: int, steps: int, warmup: int) -> dict:
    import bench_init as BI
    from tests import oracle_bcq as OB
    from tests import oracle_crr as OC
    from tianshou_amd import bcq as BQ
    from tianshou_amd import crr as CR

    p = OC.init_params(C, H, W, N_ACT, 0)
    crr = CR.CRREngine(C, H, W, N_ACT, CR.flat_from_torch([p[k] for k in OC.PARAM_ORDER], C, H, W, N_ACT),
                       CR.CRRConfig(gamma=GAMMA, policy_improvement_mode=MODE, beta=BETA, ratio_upper_bound=RATIO_UPPER_BOUND,
                                    min_q_weight=MIN_Q_WEIGHT, target_update_freq=FREQ, lr=LR))
    pb = OB.init_params(C, H, W, N_ACT, 0)
    bcq = BQ.BCQEngine(C, H, W, N_ACT, BQ.flat_from_torch([pb[k] for k in OB.PARAM_ORDER], C, H, W, N_ACT),
                       BQ.BCQConfig(gamma=GAMMA, n_step=1, target_update_freq=FREQ, unlikely_action_threshold=TAU,
                                    imitation_logits_penalty=THETA, lr=LR))
    eager = _eager()
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randint(0, 256, (batch, H, W, C), generator=g, device="cuda", dtype=torch.uint8)
    obs_next = torch.randint(0, 256, (batch, H, W, C), generator=g, device="cuda", dtype=torch.uint8)
    obs_nchw, obs_next_nchw = (x.permute(0, 3, 1, 2).contiguous() for x in (obs, obs_next))
    act = torch.randint(0, N_ACT, (batch,), generator=g, device="cuda")
    rew = torch.randn(batch, generator=g, device="cuda")
    done = (torch.rand(batch, generator=g, device="cuda") < 0.05).to(torch.uint8)
    mask = 1.0 - done.float()
    ret = rew.clone()

    def crr_update():
        return crr.update_with_batch(obs, obs_next, act, rew, done).tolist()

    def bcq_target():
        ret.copy_(rew + GAMMA * mask * bcq.target_q(obs_next))
        return None

    def bcq_update():
        return bcq.update_with_batch(obs, act, ret).tolist()

    def bcq_both():
        bcq_target()
        return bcq_update()

    def eager_update():
        return eager(obs_nchw, obs_next_nchw, act, rew, done)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    BI.warm_clocks()
    n, warm = max(steps, 20), max(warmup, 3)
    order = [(crr_update, []), (bcq_both, []), (bcq_target, []), (bcq_update, []), (eager_update, [])]
    last = None
    for i in range(warm + n):
        k = i % len(order)
        for fn, sink in order[k:] + order[:k]:                      # rotate who goes first
            dt, out = timed(fn)
            if i >= warm:
                sink.append(dt)
            if fn is crr_update:
                last = out
    sc, sboth, st, su, se = (_stats(t) for _, t in order)
    return {"batch": batch, "crr_update": sc, "bcq_target_q_plus_update": sboth, "bcq_target_q": st, "bcq_update": su,
            "eager_same_gpu": se, "timed_updates": n, "warmup": warm,
            "crr_ms": sc["ms_per_update_median"], "bcq_target_q_plus_update_ms": sboth["ms_per_update_median"],
            "bcq_target_q_ms_plus_update_ms": st["ms_per_update_median"] + su["ms_per_update_median"],
            "crr_ms_over_bcq_ms": sc["ms_per_update_median"] / sboth["ms_per_update_median"],
            "crr_vs_eager": sc["updates_per_s_median"] / se["updates_per_s_median"],
            "crr_not_slower_than_eager": sc["ms_per_update_median"] <= se["ms_per_update_median"],
            "final_losses": last, "parameters": crr.P}


def run_class_level(batch: int, steps: int, warmup: int) -> dict:
    """HipDiscreteCRR.update() over the stand-ins and a host buffer of 5,000 transitions in 10 sub-buffers: updates/s with the
    placeholder preprocessing and with the host discounted-return computation of the reference's base `_preprocess_batch`."""
    from oracle import oracle as O
    from tests import standin_crr as SC
    from tianshou_amd.integration import make_hip_discrete_crr

    class WithHostReturns(SC.DiscreteCRR):
        """add_discounted_returns (modelfree/reinforce.py:273-312) on the host: v_s_ = the running mean, lambda = 1."""

        def _preprocess_batch(self, batch, buffer, indices):
            drc = self.discounted_return_computation
            v_s_ = np.full(indices.shape, drc.ret_rms.mean)
            batch.returns, _ = O.compute_episodic_return(batch.rew, batch.terminated, batch.truncated, indices,
                                                         buffer.unfinished_index(), v_s_, None, drc.gamma, 1.0)
            return batch

    E, slots = 10, 500
    rng = np.random.default_rng(3)
    buf = SC.VectorReplayBuffer(E * slots, E, obs_shape=(C, H, W), act_shape=(), obs_dtype=np.uint8, act_dtype=np.int64)
    buf.obs[:] = rng.integers(0, 256, size=buf.obs.shape, dtype=np.uint8)
    buf.obs_next[:] = rng.integers(0, 256, size=buf.obs.shape, dtype=np.uint8)
    buf.act[:] = rng.integers(0, N_ACT, size=buf.act.shape)
    buf.rew[:] = rng.normal(size=buf.rew.shape)
    buf.terminated[:] = rng.random(buf.rew.shape) < 0.01
    buf.done[:] = buf.terminated
    for e, sb in enumerate(buf.buffers):
        sb._size, sb._insertion_idx = slots, 0
        buf._lengths[e] = slots
        buf.last_index[e] = buf._offset[e] + slots - 1
    out = {}
    for name, base in (("placeholder_preprocess", SC.DiscreteCRR), ("host_discounted_returns", WithHostReturns)):
        ns = type("ns", (), dict(vars(SC)))
        ns.DiscreteCRR = base
        torch.manual_seed(0)
        trunk = SC.DQNetFeaturesOnly(C, H, W)
        actor = SC.DiscreteActor(preprocess_net=trunk, action_shape=N_ACT, hidden_sizes=[512], softmax_output=False)
        critic = SC.DiscreteCritic(preprocess_net=trunk, hidden_sizes=[512], last_size=N_ACT)
        algo = make_hip_discrete_crr(ref=ns)(policy=SC.DiscreteActorPolicy(actor=actor), critic=critic, lr=LR, gamma=GAMMA,
                                             policy_improvement_mode=MODE, ratio_upper_bound=RATIO_UPPER_BOUND, beta=BETA,
                                             min_q_weight=MIN_Q_WEIGHT, target_update_freq=FREQ, device="cuda").to("cuda")
        algo.policy.is_within_training_step = True
        times = []
        for i in range(max(warmup, 3) + max(steps, 20)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            algo.update(buf, batch)
            torch.cuda.synchronize()
            if i >= max(warmup, 3):
                times.append(time.perf_counter() - t0)
        out[name] = _stats(times)
    out["host_preprocess_ms"] = (out["host_discounted_returns"]["ms_per_update_median"]
                                 - out["placeholder_preprocess"]["ms_per_update_median"])
    return out


def run(steps: int, warmup: int) -> dict:
    big, small = run_batch(512, steps, warmup), run_batch(32, steps, warmup)
    cls = {"B512": run_class_level(512, steps, warmup), "B32": run_class_level(32, steps, warmup)}
    return {
        "metric": "DiscreteCRR engine-level updates/sec (B=512, NatureCNN trunk, actor + critic heads, lagged pair, exp mode)",
        "value": big["crr_update"]["updates_per_s_median"], "unit": "updates/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic",
        "higher_is_better": True,
        "config": {"workload": f"C3-shape DiscreteCRR: u8[84,84,4] observations, {N_ACT} actions, B=512 and B=32, mode {MODE}, "
                               f"beta {BETA}, ratio_upper_bound {RATIO_UPPER_BOUND}, min_q_weight {MIN_Q_WEIGHT}, target sync every "
                               f"{FREQ}; one update = live pass + lagged pass + loss + backward + Adam",
                   "bcq": "the DiscreteBCQ engine on the same inputs: target_q + update (its second network pass is in preprocessing)",
                   "eager": "the same CRR update on tests/standin_crr.py modules on the same GPU, torch.optim.Adam, fp32",
                   "class_level": "HipDiscreteCRR.update() over stand-ins and a host buffer (sampling, mirror sync, gathers "
                                  "included), without and with the base class's host discounted returns"},
        "B512": big, "B32": small, "class_level": cls,
        "conditions": {"crr_not_slower_than_eager": bool(big["crr_not_slower_than_eager"] and small["crr_not_slower_than_eager"])},
    }


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crr_bench.json"))
    a = ap.parse_args()
    res = run(a.steps, a.warmup)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    if not res["conditions"]["crr_not_slower_than_eager"]:
        sys.exit("DiscreteCRR engine is slower than the eager update")
