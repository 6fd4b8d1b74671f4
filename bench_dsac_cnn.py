"""DiscreteSAC on the Atari trunk (record, not a gate): 84x84x4 uint8 observations, 6 actions, AutoAlpha, at B = 64 (the batch
size of examples/atari/atari_sac.py) and at B = 512 -- the engine beside the same update in eager PyTorch on the same GPU, in
one process.

    python bench_dsac_cnn.py [--steps K] [--warmup W] [--out profiles/dsac_cnn_bench.json]

One "update" = `target_q` on the next observations (the live trunk + actor head, the lagged trunk + both lagged critic heads,
the soft state value), the one-step return, and the update proper: three trunk forward + backward passes on the
observations, each with its own Adam step over trunk + own head, in sequence (critic 1, critic 2, actor), AutoAlpha's step
and the Polyak step of the lagged vector.  The eager baseline is the reference's update (discrete_sac.py:147-196) written out
below on the stand-in modules of tests/standin_dsac_cnn.py moved to the device, with three torch.optim.Adam instances that
all hold the shared trunk, and two lagged deep copies.  Both are timed in alternation, each call on its own with a device
synchronisation, after a clock warm-up; the figure is the median of the timed calls.  No ratio is fixed in advance; one
condition is checked: the engine must not be slower than the eager update.  Prints one JSON line and writes it to --out.
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

C, H, W, N_ACT, HIDDEN = 4, 84, 84, 6, 512
GAMMA, TAU, ACTOR_LR, CRITIC_LR, ALPHA_LR = 0.99, 0.005, 1e-5, 1e-5, 3e-4        # atari_sac.py's defaults
TARGET_ENTROPY, LOG_ALPHA0 = 0.98 * float(np.log(N_ACT)), 0.0


def _stats(times: list[float]) -> dict:
    med = statistics.median(times)
    q = statistics.quantiles(times, n=4)
    return {"updates_per_s_median": 1.0 / med, "updates_per_s_min": 1.0 / max(times), "updates_per_s_max": 1.0 / min(times),
            "ms_per_update_median": med * 1e3, "ms_per_update_q1": q[0] * 1e3, "ms_per_update_q3": q[2] * 1e3}


def _eager():
    """The reference's target and update restated on the stand-in modules -> a callable (obs, obs_next NCHW uint8)."""
    import copy

    from torch.distributions import Categorical

    from tests import standin_dsac_cnn as SD

    torch.manual_seed(0)
    net = SD.DQNet(C, H, W, action_shape=N_ACT, features_only=True, output_dim_added_layer=HIDDEN)
    actor = SD.DiscreteActor(preprocess_net=net, action_shape=N_ACT, softmax_output=False).cuda()
    critic1 = SD.DiscreteCritic(preprocess_net=net, last_size=N_ACT).cuda()
    critic2 = SD.DiscreteCritic(preprocess_net=net, last_size=N_ACT).cuda()
    critic1_old, critic2_old = copy.deepcopy(critic1), copy.deepcopy(critic2)
    opt_a = torch.optim.Adam(actor.parameters(), lr=ACTOR_LR)
    opt_1 = torch.optim.Adam(critic1.parameters(), lr=CRITIC_LR)
    opt_2 = torch.optim.Adam(critic2.parameters(), lr=CRITIC_LR)
    log_alpha = torch.nn.Parameter(torch.tensor(LOG_ALPHA0, device="cuda"))
    opt_alpha = torch.optim.Adam([log_alpha], lr=ALPHA_LR)

    def step(opt, loss):
        opt.zero_grad()
        loss.backward()
        opt.step()

    def one(obs, obs_next, act, rew, mask):
        alpha = log_alpha.detach().exp().item()
        with torch.no_grad():
            dist = Categorical(logits=actor(obs_next)[0])
            tq = (dist.probs * torch.min(critic1_old(obs_next), critic2_old(obs_next))).sum(-1) + alpha * dist.entropy()
            target_q = rew + GAMMA * mask * tq
        a = act.unsqueeze(1)
        td1 = critic1(obs).gather(1, a).flatten() - target_q
        c1 = td1.pow(2).mean()
        step(opt_1, c1)
        td2 = critic2(obs).gather(1, a).flatten() - target_q
        c2 = td2.pow(2).mean()
        step(opt_2, c2)
        weight = (td1 + td2) / 2.0
        dist = Categorical(logits=actor(obs)[0])
        entropy = dist.entropy()
        with torch.no_grad():
            q = torch.min(critic1(obs), critic2(obs))
        al = -(alpha * entropy + (dist.probs * q).sum(dim=-1)).mean()
        step(opt_a, al)
        a_loss = -(log_alpha * (TARGET_ENTROPY - entropy.detach())).mean()
        step(opt_alpha, a_loss)
        with torch.no_grad():
            for old, new in ((critic1_old, critic1), (critic2_old, critic2)):
                for po, pn in zip(old.parameters(), new.parameters()):
                    po.copy_(TAU * pn + (1 - TAU) * po)
        return torch.stack([al.detach(), c1.detach(), c2.detach(), log_alpha.detach().exp(), a_loss.detach()]).tolist(), weight

    return one


def run_batch(batch: int, steps: int, warmup: int) -> dict:
    import bench_init as BI
    from tests import oracle_dsac_cnn as OS
    from tianshou_amd import dsac_cnn as DS
    from tianshou_amd.sac import SACConfig

    p = OS.init_params(C, H, W, N_ACT, HIDDEN, 0)
    cfg = SACConfig(gamma=GAMMA, tau=TAU, n_step=1, auto_alpha=True, target_entropy=TARGET_ENTROPY, log_alpha0=LOG_ALPHA0,
                    actor_lr=ACTOR_LR, critic_lr=CRITIC_LR, alpha_lr=ALPHA_LR)
    eng = DS.DiscreteSACCnnEngine(C, H, W, N_ACT, HIDDEN, DS.flat_from_torch([p[k] for k in OS.PARAM_ORDER], C, H, W, N_ACT, HIDDEN), cfg)
    eager = _eager()
    g = torch.Generator(device="cuda").manual_seed(2)
    obs = torch.randint(0, 256, (batch, H, W, C), generator=g, device="cuda", dtype=torch.uint8)
    obs_next = torch.randint(0, 256, (batch, H, W, C), generator=g, device="cuda", dtype=torch.uint8)
    obs_nchw, obs_next_nchw = (x.permute(0, 3, 1, 2).contiguous() for x in (obs, obs_next))
    act = torch.randint(0, N_ACT, (batch,), generator=g, device="cuda")
    rew = torch.randn(batch, generator=g, device="cuda")
    mask = 1.0 - (torch.rand(batch, generator=g, device="cuda") < 0.05).float()

    def engine_update():
        ret = rew + GAMMA * mask * eng.target_q(obs_next)
        stats, _ = eng.update_with_batch(obs, act, ret)
        return stats.tolist()

    def eager_update():
        return eager(obs_nchw, obs_next_nchw, act, rew, mask)[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    BI.warm_clocks()
    n, warm = max(steps, 20), max(warmup, 3)
    order = [(engine_update, []), (eager_update, [])]
    last = None
    for i in range(warm + n):
        k = i % len(order)
        for fn, sink in order[k:] + order[:k]:                      # rotate who goes first
            dt, out = timed(fn)
            if i >= warm:
                sink.append(dt)
            if fn is engine_update:
                last = out
    se, sg = (_stats(t) for _, t in order)
    return {"batch": batch, "engine_target_q_plus_update": se, "eager_same_gpu": sg, "timed_updates": n, "warmup": warm,
            "engine_ms": se["ms_per_update_median"], "eager_ms": sg["ms_per_update_median"],
            "engine_vs_eager": se["updates_per_s_median"] / sg["updates_per_s_median"],
            "engine_not_slower_than_eager": se["ms_per_update_median"] <= sg["ms_per_update_median"],
            "final_stats": last, "parameters": eng.P}


def run(steps: int, warmup: int) -> dict:
    small, big = run_batch(64, steps, warmup), run_batch(512, steps, warmup)
    return {
        "metric": "DiscreteSAC-on-the-Atari-trunk engine-level updates/sec (B=64, one shared NatureCNN trunk + added layer, "
                  "actor + two critic heads, three optimizers, AutoAlpha)",
        "value": small["engine_target_q_plus_update"]["updates_per_s_median"], "unit": "updates/s", "n_gpus": 1, "dtype": "f32",
        "data": "synthetic", "higher_is_better": True,
        "config": {"workload": f"atari_sac.py shape: u8[84,84,4] observations, {N_ACT} actions, hidden {HIDDEN}, B=64 and B=512, "
                               f"tau {TAU}, lr {ACTOR_LR} / {CRITIC_LR} / {ALPHA_LR}; one update = target_q on obs_next + three "
                               "trunk forward/backward passes with three Adam steps + alpha + Polyak",
                   "eager": "the same target and update on tests/standin_dsac_cnn.py modules on the same GPU, three "
                            "torch.optim.Adam over the shared trunk, fp32"},
        "B64": small, "B512": big,
        "conditions": {"engine_not_slower_than_eager": bool(small["engine_not_slower_than_eager"] and big["engine_not_slower_than_eager"])},
    }


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsac_cnn_bench.json"))
    a = ap.parse_args()
    res = run(a.steps, a.warmup)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    if not res["conditions"]["engine_not_slower_than_eager"]:
        sys.exit("the DiscreteSAC engine is slower than the eager update")
