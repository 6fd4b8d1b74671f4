"""Binding a Tianshou maintainer adds: `HipPPO`, a `PPO` subclass whose learn() hooks run on the
MI355X engine.  Needs `tianshou` importable (it is not on the GPU test box; there the same engine
is driven through `tianshou_amd.ppo.PPOEngine` directly).

Overrides exactly the two hooks `Algorithm._update` calls (algorithm_base.py:622-627):
    _preprocess_batch(batch, buffer, indices) -> batch          (ppo.py:146-162)
    _update_with_batch(batch, batch_size, repeat) -> A2CTrainingStats   (ppo.py:164-224)
keeping the Policy / Algorithm API, the Batch fields (`v_s`, `returns`, `adv`, `logp_old`, `act`),
the stats dataclasses and `state_dict()` (parameters and Adam moments are copied back into the
torch modules / optimizer after every update(), or, under `write_back="lazy"`, when somebody reads them; for the
Q-learning classes, HipDQN to HipRainbow, that copy is `_q_write_back`; for the off-policy actor-critic classes, HipSAC, HipREDQ,
HipDiscreteSAC and HipTD3 / HipDDPG / HipTD3BC, it is `_ac_write_back`; for the on-policy classes, HipPPO to HipPPODiscrete and their A2C
variants, it is `_on_write_back`, and HipPPO's Adam moments alone wait for a reader).  Supported net: the MuJoCo actor-critic of
examples/mujoco/mujoco_ppo.py (Net[64,64] tanh, ContinuousActorProbabilistic(unbounded=True) with a
state-independent sigma, ContinuousCritic); anything else raises at construction.
"""
from __future__ import annotations

import os
import weakref
from typing import Callable, NamedTuple

import numpy as np
import torch

from .checkpoint import adam_state, params_by_keys, store_adam_state
from .ppo import PPOConfig, PPOEngine, flat_from_modules, flat_to_modules, TIANSHOU_ACTOR_KEYS, TIANSHOU_CRITIC_KEYS


def _algorithm_state_loaded(module, incompatible_keys) -> None:
    """load_state_dict post-hook of the Hip* algorithms (module level, so that the algorithm stays picklable)."""
    module._hip_invalidate()


# Sub-modules of an algorithm with lazy write-back -> that algorithm.  `actor.state_dict()` / `torch.save(critic.state_dict())`
# on a SUB-module reads torch parameters the engine may be ahead of; a state_dict pre-hook on every sub-module syncs first.
# The hook is a module-level function (picklable by reference) and finds its owner through this process-local weak table, so
# the modules carry no closure; in another process (an unpickled copy) the lookup misses and the hook is a no-op.
_LAZY_OWNERS: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()


def _sync_owner_before_state_dict(module, prefix, keep_vars) -> None:
    owner = _LAZY_OWNERS.get(id(module))
    # (the table is keyed by id(): an entry may outlive its module -- a replaced sub-module whose id a foreign module took over --
    # so the owner is asked whether the module is still one of its own)
    if owner is not None and not owner.__dict__.get("_hip_in_update", False) and any(m is module for m in owner.modules()):
        owner.hip_sync()


class _HipGlue:
    """Mixed in (first base) by every Hip* subclass: the two places where the torch-side state of the
    reference moves underneath an engine that snapshotted it.

    * Learning rates.  `Algorithm._update` steps every scheduler after each update()
      (algorithm_base.py:516-518, 628-629; `LambdaLR` only rewrites `param_groups[i]["lr"]`, optim.py:22-53) and
      examples/mujoco/mujoco_ppo.py:124-131 turns linear decay on by default.  The engines rebuild their
      hyper-parameter struct from `eng.cfg` on every call, so `_hip_refresh_lr()` at the top of each
      `_update_with_batch` re-reads the optimizers' current values.
    * `load_state_dict` on the algorithm replaces parameters / Adam moments / lagged networks / counters: the engine
      is dropped and rebuilt from the loaded torch state on the next update.  A load into a sub-module
      (`algorithm.policy.load_state_dict(best)`) replaces parameters only: it is noticed through the parameters'
      version counters, the engine's Adam moments are first written into torch.optim and survive the rebuild.  Under lazy
      write-back the same check runs in front of every reader (`hip_sync()`, `state_dict()`, pickling the policy): the
      loaded module keeps what was loaded, every other module gets what the engine learnt.
    Only writes that bump a tensor's version counter are seen (`load_state_dict`, `param.copy_()`, in-place ops on the
    Parameter); writes through `param.data` (`param.data.copy_()`, optimizer-style `param.data.add_()`, `module.to()`) do
    NOT bump it -- call `algorithm.hip_sync()` before such an edit and `algorithm.hip_invalidate()` after it
    (`hip_invalidate()` raises while lazy updates are pending).  A sub-module REPLACED after the engine was built
    (`algorithm.policy.actor = new`) is not seen either: the same two calls go around the replacement.
    `_HIP_LR`: (engine cfg field, attribute path of the Algorithm.Optimizer wrapper that owns it)."""
    _HIP_LR: tuple = (("lr", "optim"),)
    _hip_dp_on = False            # classes whose constructor takes data_parallel= call _hip_dp_setup

    def _hip_glue_init(self) -> None:
        # Only the algorithm itself carries a hook, and it is a module-level function: sub-modules stay free of
        # closures so that `torch.save(policy)` / `pickle.dumps(algorithm.policy)` (highlevel/persistence.py:106)
        # and `copy.deepcopy(policy)` keep working.  Loads into sub-modules are caught by the version check below.
        self.register_load_state_dict_post_hook(_algorithm_state_loaded)

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        f = cls.__dict__.get("_update_with_batch")
        if f is not None and not getattr(f, "_hip_wrapped", False):
            import functools

            @functools.wraps(f)
            def _update_with_batch(self, *a, **k):
                self.__dict__["_hip_in_update"] = True      # our own write-back must not look like a foreign write
                try:
                    out = f(self, *a, **k)
                finally:
                    self.__dict__["_hip_in_update"] = False
                self._hip_mark()          # the engine has just written the parameters back: that is "our" version
                return out

            _update_with_batch._hip_wrapped = True
            cls._update_with_batch = _update_with_batch

    # The engine snapshots the torch parameters.  `_hip_engine` is a property so that every access first checks
    # whether somebody else has written them since (`algorithm.policy.load_state_dict(best)`,
    # `actor.load_state_dict(...)`, an in-place edit): tensor `_version` counters of all parameters.  If so, the
    # engine-side Adam moments are flushed into torch.optim (they are still valid: only parameters were replaced) and
    # the engine is rebuilt from the torch state on the next use.
    def _hip_current_versions(self) -> tuple:
        # the modules' own `_parameters` dicts, collected once per engine (walking `self.parameters()` costs 0.16 ms on a SAC
        # algorithm and runs on every hook); a Parameter object replaced inside a module is still seen (the dict is live), a
        # sub-module added afterwards is not -- `hip_invalidate()` covers that
        dicts = self.__dict__.get("_hip_pdicts")
        if dicts is None:
            dicts = self.__dict__["_hip_pdicts"] = [m._parameters for m in self.modules() if m._parameters]
        return tuple((id(p), p._version) for d in dicts for p in d.values() if p is not None)

    def _hip_mark(self) -> None:
        if self.__dict__.get("_hip_engine_obj") is not None and not self.__dict__.get("_hip_clean_mark", False):
            self.__dict__["_hip_versions"] = self._hip_current_versions()
        self.__dict__["_hip_clean_mark"] = False

    @property
    def _hip_engine(self):
        eng = self.__dict__.get("_hip_engine_obj")
        if eng is not None and not self.__dict__.get("_hip_in_update", False):
            seen = self.__dict__.get("_hip_versions")
            if seen is not None:
                now = self._hip_current_versions()
                if seen != now:
                    self.__dict__["_hip_versions"] = None          # (the flush reads `_hip_engine` itself: no re-entry)
                    if self.__dict__.get("_hip_stale", False):
                        # lazy write-back: what the engine learnt since the last sync goes to every parameter that was NOT
                        # written by somebody else (theirs wins), then the engine is rebuilt from the torch state
                        old = dict(seen)
                        self.__dict__["_hip_skip_ids"] = {i for i, v in now if old.get(i, v) != v} | (set(dict(now)) - set(old))
                        try:
                            self._hip_write_back()
                        finally:
                            self.__dict__["_hip_skip_ids"] = None
                            self.__dict__["_hip_stale"] = False
                    self._hip_flush()
                    self.__dict__["_hip_engine_obj"] = eng = None
                    self._hip_adam_dirty = False
        return eng

    @_hip_engine.setter
    def _hip_engine(self, value) -> None:
        self.__dict__["_hip_engine_obj"] = value
        self.__dict__["_hip_pdicts"] = self.__dict__["_hip_modules"] = self.__dict__["_hip_ac_params"] = None
        self.__dict__["_hip_versions"] = None if value is None else self._hip_current_versions()

    # -- write-back of what the engine learnt (off-policy subclasses) ---------------------------------------------------
    # "eager": after every update (the torch modules are always current: what round 5 did).  "lazy": when somebody reads
    # them -- `state_dict()` of the algorithm or of the attached policy, pickling, `hip_sync()`, a foreign write, a
    # rebuild.  The collector does not: with `policy_forward="hip"` it acts with the engine's parameters
    # (tianshou_amd/policy.py).  An eager write-back is ~600 small torch ops (2 ms per SAC update against 0.36 ms of GPU work).
    def _hip_put(self, p, t) -> None:
        skip = self.__dict__.get("_hip_skip_ids")
        if skip and id(p) in skip:
            return
        p.copy_(t.reshape(p.shape) if t.shape != p.shape else t)

    def _hip_write_back(self) -> None:
        """Engine parameters / lagged parameters / optimizer state -> the torch modules (subclasses with lazy write-back)."""

    def _hip_after_update(self) -> None:
        if self.__dict__.get("_hip_lazy", False):
            self.__dict__["_hip_stale"] = True
            self.__dict__["_hip_clean_mark"] = True          # nothing was written to the torch parameters: the mark stands
        else:
            self._hip_write_back()

    def hip_sync(self) -> None:
        """Public: make the torch modules and optimizers current (no-op unless updates are pending under write_back="lazy").
        A foreign write since the last sync (`policy.load_state_dict(best)`) is honoured first: the `_hip_engine` property
        writes what the engine learnt to every OTHER parameter, flushes the optimizer state and drops the engine."""
        self._hip_engine                                  # noqa: B018 (the version check of the property)
        if self.__dict__.get("_hip_stale", False) and self.__dict__.get("_hip_engine_obj") is not None:
            self.__dict__["_hip_stale"] = False
            self.__dict__["_hip_in_update"] = True
            try:
                self._hip_write_back()
            finally:
                self.__dict__["_hip_in_update"] = False
            self.__dict__["_hip_versions"] = self._hip_current_versions()

    def _hip_set_write_back(self, write_back: str, attached: bool) -> None:
        if write_back not in ("auto", "lazy", "eager"):
            raise ValueError("write_back must be 'auto', 'lazy' or 'eager'")
        self.__dict__["_hip_lazy"] = write_back == "lazy" or (write_back == "auto" and attached)
        if self.__dict__["_hip_lazy"]:
            for m in self.modules():                      # (the algorithm's own state_dict() / hip_sync() are overridden)
                if m is self:
                    continue
                _LAZY_OWNERS[id(m)] = self                # (latest owner wins: a stale entry under a recycled id is replaced)
                if _sync_owner_before_state_dict not in m._state_dict_pre_hooks.values():
                    m.register_state_dict_pre_hook(_sync_owner_before_state_dict)

    def _hip_offpolicy_update(self, buffer, sample_size, Batch, TrainingStats=None):
        """`OffPolicyAlgorithm.update` -> `Algorithm._update` (algorithm_base.py:586-631, 893-903): the same steps in the same
        order, except that `buffer.sample(sample_size)` -- `sample_indices` + a host fancy-index copy of every key of the batch
        (1.5 ms for 4,096 Humanoid transitions) -- keeps only its first half: the hooks read the rows from the device mirror
        by index.  A prioritized buffer's importance weights are attached as its `__getitem__` does (prio.py:103-106)."""
        import time

        if not self.policy.is_within_training_step:
            raise RuntimeError(
                f"update() was called outside of a training step as signalled by {self.policy.is_within_training_step=} "
                "(see tianshou.utils.torch_utils.policy_within_training_step)")
        if buffer is None:
            return TrainingStats() if TrainingStats is not None else None
        start = time.time()
        indices = buffer.sample_indices(sample_size)
        batch = Batch()
        if hasattr(buffer, "get_weight"):
            w = buffer.get_weight(indices)
            batch.weight = w / np.max(w) if getattr(buffer, "_weight_norm", True) else w
        self.__dict__["_hip_own_sequence"] = True        # (HipSAC: preprocess + update of an n_step = 1 batch become one library call)
        try:
            batch = self._preprocess_batch(batch, buffer, indices)
        finally:
            self.__dict__["_hip_own_sequence"] = False
        # torch_train_mode (torch_utils.py:14-22) is `train(True)` ... `train(was_training)` around the update; the engine reads
        # no module flag, so only the second call is observable: every sub-module ends in the algorithm's mode.  `train()` walks
        # ~60 modules through `Module.__setattr__` (0.24 ms); reading their flags costs 5 us and is almost always enough
        was_training = self.training
        try:
            stat = self._update_with_batch(batch)
        finally:
            mods = self.__dict__.get("_hip_modules")
            if mods is None:
                mods = self.__dict__["_hip_modules"] = list(self.modules())
            if any(m.training != was_training for m in mods):
                self.train(was_training)
        self._postprocess_batch(batch, buffer, indices)
        for lr_scheduler in self.lr_schedulers:
            lr_scheduler.step()
        stat.train_time = time.time() - start
        return stat

    # -- data parallelism: one process per GPU, the replay buffer sharded by sub-buffer (env id), one
    # all-reduce of the flat gradient per minibatch step; replaces the reference's single-process nn.DataParallel
    # (utils/net/common.py:473-515).  `_hip_dp_setup` is called by the constructors that take `data_parallel=`.
    def _hip_dp_setup(self, data_parallel: bool, group, allreduce, shard_buffer: bool) -> None:
        self._hip_dp_on = bool(data_parallel)
        self._hip_group = group
        self._hip_allreduce = allreduce          # None: torch.distributed; "native": NativeAllReduce; or a callable
        self._hip_shard = bool(shard_buffer) and self._hip_dp_on
        self._hip_dp_obj = None

    def _hip_world(self) -> tuple[int, int]:
        import torch.distributed as dist

        if not getattr(self, "_hip_dp_on", False) or not dist.is_initialized():
            return 0, 1
        return dist.get_rank(self._hip_group), dist.get_world_size(self._hip_group)

    def _hip_shard_range(self, buffer):
        """This rank's sub-buffers of `buffer` (None: mirror everything)."""
        rank, world = self._hip_world()
        if not getattr(self, "_hip_shard", False) or world == 1:
            return None
        from .distributed import shard_envs

        n_env = len(buffer.buffers) if hasattr(buffer, "buffers") else 1
        if n_env < world:
            raise ValueError(f"cannot shard {n_env} sub-buffers over {world} ranks")
        return shard_envs(n_env, rank, world)

    def _hip_dp(self, wrapper_cls, eng):
        """The DataParallel* wrapper around the current engine (rebuilt when the engine is)."""
        obj = self._hip_dp_obj
        if obj is None or obj.eng is not eng:
            ar = self._hip_allreduce
            if ar == "native":
                from .collective import NativeAllReduce

                ar = self.__dict__.get("_hip_native_ar")
                if ar is None:
                    ar = self.__dict__["_hip_native_ar"] = NativeAllReduce(self._hip_device, group=self._hip_group)
            obj = self._hip_dp_obj = wrapper_cls(eng, group=self._hip_group, allreduce=ar)
        return obj

    def _hip_invalidate(self) -> None:
        """`Algorithm.load_state_dict` replaced parameters AND optimizer state: drop the engine without flushing."""
        self.__dict__["_hip_engine_obj"] = None
        self.__dict__["_hip_versions"] = None
        self.__dict__["_hip_pdicts"] = self.__dict__["_hip_modules"] = self.__dict__["_hip_ac_params"] = None
        self.__dict__["_hip_stale"] = False
        self._hip_adam_dirty = False
        # the collector forward's flat copy of the torch parameters is keyed on (data_ptr, _version): blind to `.data` edits too
        pol = self.__dict__.get("_modules", {}).get("policy")
        if pol is not None:
            pol.__dict__.pop("_hip_rt_flat", None)

    def hip_invalidate(self, keep_optimizer: bool = True) -> None:
        """Public: the torch parameters were edited in a way the version check cannot see (`param.data` writes, `.to()`):
        drop the engine so that the next update (and the collector forward) rebuilds it from the torch state.
        keep_optimizer=True first writes the engine's Adam moments / step counters into torch.optim (they survive the
        rebuild); False discards them and writes nothing (use after replacing the optimizer state yourself).
        Under lazy write-back the engine may hold updates the torch modules do not have yet, and an edit through `.data`
        cannot be told apart from them: with updates pending this raises (nothing is dropped, nothing is written).  The
        recipe is `hip_sync()`, then the edit, then `hip_invalidate()`; when the edit replaces the optimizer state too
        (`optim.load_state_dict(o)`, then `hip_invalidate(keep_optimizer=False)`), `hip_sync()` comes before it, since
        the sync writes the engine's moments into torch.optim."""
        if keep_optimizer:
            self._hip_engine                              # noqa: B018 (a version-visible foreign write is honoured first)
        if self.__dict__.get("_hip_stale", False) and self.__dict__.get("_hip_engine_obj") is not None:
            raise RuntimeError(f"{type(self).__name__}.hip_invalidate(): updates are pending in the engine (lazy write-back) and "
                               "would be lost; call hip_sync() BEFORE editing parameters through `.data` or replacing the "
                               "optimizer state, then hip_invalidate()")
        if keep_optimizer and self.__dict__.get("_hip_engine_obj") is not None:
            self.__dict__["_hip_versions"] = None
            self._hip_flush()
        self._hip_invalidate()

    def _hip_flush(self) -> None:
        """Engine-side optimizer state -> torch.optim state; the default wrappers store it after every update."""

    def state_dict(self, *args, **kwargs):
        self.hip_sync()
        self._hip_flush()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, *args, **kwargs):
        # lazy write-back: pending updates reach the torch state first, so that what the checkpoint does not replace keeps what
        # the engine learnt, as under eager write-back (AutoAlpha's optimizer lives outside Algorithm._optimizers, sac.py:193)
        self.hip_sync()
        return super().load_state_dict(state_dict, *args, **kwargs)

    def _hip_refresh_lr(self) -> None:
        eng = self._hip_engine
        if eng is None:
            return
        seen: dict[str, float] = {}
        for field, path in self._HIP_LR:
            obj = self
            for part in path.split("."):
                obj = getattr(obj, part)
            opt = getattr(obj, "_optim", obj)
            if not hasattr(opt, "param_groups"):          # FixedAlpha (sac.py:161-172): nothing to learn
                continue
            lr = float(opt.param_groups[0]["lr"])
            if any(float(g["lr"]) != lr for g in opt.param_groups):
                raise NotImplementedError("the HIP engines take one learning rate per optimizer")
            if seen.setdefault(field, lr) != lr:
                raise NotImplementedError(f"the HIP engine has one `{field}`; the optimizers sharing it disagree")
            setattr(eng.cfg, field, lr)
            opt._opt_called = True       # the engine performs this optimizer's step (LRScheduler.step's order check)


def _policy_extra_state(algorithm) -> dict:
    """The run state of the attached collector forward (tianshou_amd/policy.py) that no state_dict() holds: the call counter of
    its device sampling noise.  Saved by `hip_extra_state()` so that a resumed run continues the noise sequence."""
    return {"policy_calls": int(algorithm.policy.__dict__.get("_hip_rt_calls", 0))}


def _load_policy_extra_state(algorithm, state: dict) -> None:
    if "policy_calls" in state:                        # (extra states written before the counter was saved have none)
        algorithm.policy.__dict__["_hip_rt_calls"] = int(state["policy_calls"])


def optimizer_fields(opt) -> dict:
    """The PPOConfig fields of a torch optimizer built by tianshou/algorithm/optim.py: AdamOptimizerFactory (:89-110, incl.
    weight_decay) or RMSpropOptimizerFactory (:113-140: alpha, eps, weight_decay, momentum, centered -- the optimizer of
    examples/mujoco/mujoco_a2c.py:117).  Everything else (amsgrad, maximize, other classes) raises."""
    g = opt.param_groups[0]
    name = type(opt).__name__
    if g.get("maximize", False) or g.get("amsgrad", False):
        raise NotImplementedError("the HIP engines do not implement amsgrad / maximize")
    if any(any(gi.get(k) != g.get(k) for k in g if k not in ("params", "lr", "initial_lr")) for gi in opt.param_groups):
        raise NotImplementedError("the HIP engines take one hyper-parameter set per optimizer")
    if name == "Adam":
        return dict(optimizer="adam", lr=g["lr"], betas=tuple(g["betas"]), adam_eps=g["eps"],
                    weight_decay=float(g.get("weight_decay", 0) or 0.0))
    if name == "RMSprop":
        if g.get("centered", False) and g.get("momentum", 0) > 0:
            raise NotImplementedError("RMSprop(centered=True, momentum > 0): the engines keep one auxiliary state vector")
        return dict(optimizer="rmsprop", lr=g["lr"], adam_eps=g["eps"], weight_decay=float(g.get("weight_decay", 0) or 0.0),
                    rms_alpha=float(g["alpha"]), rms_momentum=float(g.get("momentum", 0) or 0.0),
                    rms_centered=bool(g.get("centered", False)))
    raise NotImplementedError(f"the HIP engines implement torch.optim.Adam and torch.optim.RMSprop, not {name}")


def ppo_config_from(algorithm) -> PPOConfig:
    """Reads the reference PPO's hyper-parameters (ppo.py:126-144, a2c.py:95-113, optim.py:89-140) and the actor's bound
    (ContinuousActorProbabilistic.max_action / _unbounded, utils/net/continuous.py:194-231)."""
    opt = algorithm.optim._optim
    of = optimizer_fields(opt)
    is_ppo = hasattr(algorithm, "eps_clip")                  # A2C (a2c.py:187-247) has none of the clipping options
    actor = getattr(algorithm.policy, "actor", None)
    bounded = actor is not None and hasattr(actor, "_unbounded") and not actor._unbounded
    return PPOConfig(
        max_action=float(actor.max_action) if bounded else None, **of,
        algo="ppo" if is_ppo else "a2c",
        gamma=algorithm.gamma, gae_lambda=algorithm.gae_lambda, eps_clip=getattr(algorithm, "eps_clip", 0.2),
        dual_clip=getattr(algorithm, "dual_clip", None), value_clip=getattr(algorithm, "value_clip", False),
        advantage_normalization=getattr(algorithm, "advantage_normalization", False),
        recompute_advantage=getattr(algorithm, "recompute_adv", False), vf_coef=algorithm.vf_coef,
        ent_coef=algorithm.ent_coef, max_grad_norm=algorithm.optim._max_grad_norm,
        return_scaling=algorithm.return_scaling)


def _ref(ref, module: str, name: str):
    """`module.name` of the reference package - or `ref.name` when a namespace is injected: the GPU parity tests drive
    the very same hook bodies through minimal stand-ins of the reference classes (tests/standin.py), because
    /root/reference does not exist on the GPU box."""
    if ref is not None:
        return getattr(ref, name)
    import importlib

    return getattr(importlib.import_module(module), name)


def _on_policy_base(algo: str, ref=None):
    """PPO (ppo.py) or A2C (a2c.py:187-290): the hooks and the statistics class are the same."""
    if algo == "ppo":
        return _ref(ref, "tianshou.algorithm.modelfree.ppo", "PPO")
    if algo == "a2c":
        return _ref(ref, "tianshou.algorithm.modelfree.a2c", "A2C")
    raise ValueError("algo must be 'ppo' or 'a2c'")


def _trunk_spec(net, who: str, norm: bool = False):
    """Net -> MLP -> Sequential(Linear, act, Linear, act, ...) (utils/net/common.py:90-178): -> (linear-layer key stems,
    hidden sizes, activation name).  One activation class for all layers (nn.Tanh / nn.ReLU) or none; other activations are
    outside the engine's envelope.  `norm=True` (the PPO / A2C hooks): MLP(norm_layer=nn.LayerNorm) -- Linear -> LayerNorm ->
    activation in every hidden layer (common.py:25-39) -- is accepted as well, see `_trunk_norm`; elsewhere a norm layer raises."""
    try:
        seq = list(net.preprocess.model.model)
    except AttributeError as e:
        raise NotImplementedError(f"HipPPO: unsupported {who} (no preprocess.model.model Sequential)") from e
    stems, hidden, acts, followed = [], [], set(), []
    for i, m in enumerate(seq):
        if isinstance(m, torch.nn.Linear):
            stems.append(f"preprocess.model.model.{i}")
            hidden.append(int(m.out_features))
            followed.append(False)
        elif isinstance(m, (torch.nn.Tanh, torch.nn.ReLU)):
            acts.add("tanh" if isinstance(m, torch.nn.Tanh) else "relu")
            if not followed or followed[-1]:
                raise NotImplementedError(f"HipPPO: {who} trunk has an activation that does not follow a Linear layer")
            followed[-1] = True
        elif isinstance(m, torch.nn.Identity):
            pass
        elif norm and isinstance(m, torch.nn.LayerNorm):
            pass                                              # (position, shape and affine-ness are checked by _trunk_norm)
        else:
            raise NotImplementedError(f"HipPPO: {who} trunk contains {type(m).__name__}; Linear layers with nn.Tanh, nn.ReLU "
                                      "or no activation are supported (nn.LayerNorm under PPO / A2C only, no other norm layers)")
    if not stems or len(acts) > 1:
        raise NotImplementedError(f"HipPPO: {who} trunk needs at least one Linear layer and a single activation class")
    # The engines apply the activation after EVERY trunk layer.  A Net built with action_shape > 0 (MLP output_dim > 0,
    # utils/net/common.py:169-170) ends in a bare Linear layer and Net(softmax=True) appends a softmax (common.py:366-367):
    # neither is a (Linear, activation) pair, so they are outside the envelope rather than silently a different network.
    if acts and not all(followed):
        raise NotImplementedError(f"HipPPO: every Linear layer of the {who} trunk must be followed by its activation "
                                  "(a Net with action_shape / MLP output_dim > 0 ends in a bare Linear layer)")
    if getattr(net.preprocess, "softmax", False):
        raise NotImplementedError(f"HipPPO: the {who} trunk applies a softmax (Net(softmax=True)); not supported")
    return stems, hidden, (acts.pop() if acts else "none")


def _trunk_norm(net, who: str):
    """-> None for a trunk without norm layers, else (key stems of the LayerNorm modules, one per Linear layer, eps): every
    Linear layer is DIRECTLY followed by an nn.LayerNorm over its own width with an elementwise affine map (weight and bias) and
    one eps for all of them -- what MLP(norm_layer=nn.LayerNorm[, norm_args]) builds (utils/net/common.py:25-39, 123-137)."""
    seq = list(net.preprocess.model.model)
    norms = [(i, m) for i, m in enumerate(seq) if isinstance(m, torch.nn.LayerNorm)]
    if not norms:
        return None
    lin = [i for i, m in enumerate(seq) if isinstance(m, torch.nn.Linear)]
    if [i for i, _ in norms] != [i + 1 for i in lin]:
        raise NotImplementedError(f"HipPPO: {who} trunk: a LayerNorm must follow every Linear layer directly (Linear -> LayerNorm "
                                  "-> activation), or none")
    eps = {float(m.eps) for _, m in norms}
    for (i, m), j in zip(norms, lin):
        if tuple(m.normalized_shape) != (seq[j].out_features,) or m.weight is None or m.bias is None:
            raise NotImplementedError(f"HipPPO: {who} trunk: LayerNorm must normalise the layer's width with weight and bias")
    if len(eps) != 1:
        raise NotImplementedError(f"HipPPO: {who} trunk: one eps for all LayerNorm modules")
    return [f"preprocess.model.model.{i}" for i, _ in norms], eps.pop()


def _ln_eps_of(hidden):
    """The ("layer_norm", eps) tag of `_check_supported`'s "net" description -> eps, or None."""
    for tag in hidden[3:] if isinstance(hidden, tuple) else ():
        if isinstance(tag, tuple) and tag[0] == "layer_norm":
            return float(tag[1])
    return None


def _net_keys(actor, critic):
    """state_dict keys of an actor / critic over Net trunks of any depth, in the engine's flat order:
    actor trunk (w, b[, gamma, beta])*, mu (w, b), sigma_param | critic trunk (w, b[, gamma, beta])*, last (w, b)."""
    def trunk(net, who):
        st, _, _ = _trunk_spec(net, who, norm=True)
        nm = _trunk_norm(net, who)
        if nm is None:
            return [f"{x}.{y}" for x in st for y in ("weight", "bias")]
        return [f"{x}.{y}" for a, b in zip(st, nm[0]) for x in (a, b) for y in ("weight", "bias")]
    ka = trunk(actor, "actor") + ["mu.model.0.weight", "mu.model.0.bias"]
    ka += ["sigma.model.0.weight", "sigma.model.0.bias"] if getattr(actor, "_c_sigma", False) else ["sigma_param"]
    kc = trunk(critic, "critic") + ["last.model.0.weight", "last.model.0.bias"]
    return ka, kc


def _check_supported(actor, critic):
    """-> (obs_dim, act_dim, hidden, kind).  kind "fused": the MuJoCo example nets (hidden 64 x 64 tanh, obs <= 31, act <= 8) on
    the fused MFMA kernels of ts_ppo.hip; "wide": any other Net[h, h] tanh (h a multiple of 32 up to 1024, act <= 32, e.g.
    Humanoid's 376 / 17 / 256 x 256) on the implicit-GEMM layer kernels (tianshou_amd/ppo_wide.py); "net": every other trunk
    the reference's Net builds from `hidden_sizes` and one activation (1 .. 7 hidden layers of any widths up to 1024, nn.Tanh /
    nn.ReLU / none, actor and critic trunks may differ) on the same layer kernels (ppo_wide.NetPPOEngine) -- `hidden` is then
    (actor hidden sizes, critic hidden sizes, activation[, "conditioned_sigma"][, ("layer_norm", eps)]): the actor's sigma is
    a second linear head (continuous.py:212-234); every hidden layer is Linear -> LayerNorm -> activation (common.py:25-39)."""
    ka, kc = _net_keys(actor, critic)
    sa, sc = actor.state_dict(), critic.state_dict()
    if set(sa.keys()) != set(ka):
        raise NotImplementedError(f"HipPPO: unsupported actor (keys {sorted(set(sa) ^ set(ka))} differ from a Net trunk + linear mu "
                                  "head + sigma_param); see tianshou_amd/integration.py")
    if set(sc.keys()) != set(kc):
        raise NotImplementedError(f"HipPPO: unsupported critic (keys {sorted(set(sc) ^ set(kc))} differ from a Net trunk + linear head)")
    # ContinuousActorProbabilistic(unbounded=False) is the constructor default (continuous.py:194): mu = max_action * tanh(.)
    # -- built into the fused step / inference kernels (ts_ppo_hparams.max_action) and into the per-layer engine
    # (ts_net_desc.max_action); the Net[h, h] GEMM engine ("wide") stays unbounded, such actors take the per-layer engine
    bounded = not getattr(actor, "_unbounded", False)
    if bounded and not float(getattr(actor, "max_action", 1.0)) > 0.0:
        raise NotImplementedError("HipPPO: a bounded actor needs max_action > 0")
    c_sigma = bool(getattr(actor, "_c_sigma", False))
    _, ha, act_a = _trunk_spec(actor, "actor", norm=True)
    _, hc, act_c = _trunk_spec(critic, "critic", norm=True)
    nm_a, nm_c = _trunk_norm(actor, "actor"), _trunk_norm(critic, "critic")
    obs_dim, act_dim = int(sa[ka[0]].shape[1]), int(sa["mu.model.0.weight"].shape[0])
    if int(sc[kc[0]].shape[1]) != obs_dim or act_a != act_c:
        raise NotImplementedError("HipPPO: actor and critic must read the same observation and use the same activation")
    if (nm_a is None) != (nm_c is None) or (nm_a is not None and nm_a[1] != nm_c[1]):
        raise NotImplementedError("HipPPO: actor and critic trunks must both have LayerNorm (one eps) or neither")
    if sa["mu.model.0.weight"].shape[1] != ha[-1] or tuple(sc["last.model.0.weight"].shape) != (1, hc[-1]):
        raise NotImplementedError("HipPPO: the heads must be single Linear layers on the trunks' outputs")
    if act_dim > (16 if c_sigma else 32):
        raise NotImplementedError("HipPPO: at most 32 actions (16 with conditioned_sigma)")
    if c_sigma and tuple(sa["sigma.model.0.weight"].shape) != (act_dim, ha[-1]):
        raise NotImplementedError("HipPPO: the sigma head must be a single Linear layer on the trunk's output")
    if nm_a is None and not c_sigma and act_a == "tanh" and ha == hc and len(ha) == 2 and ha[0] == ha[1]:
        hidden = ha[0]
        if hidden == 64 and obs_dim <= 31 and act_dim <= 8:
            return obs_dim, act_dim, hidden, "fused"
        if hidden % 32 == 0 and 32 <= hidden <= 1024 and not bounded:
            return obs_dim, act_dim, hidden, "wide"
    if max(len(ha), len(hc)) > 7 or max(ha + hc) > 1024:
        raise NotImplementedError("HipPPO: trunks of up to 7 hidden layers of at most 1024 units")
    tags = (("conditioned_sigma",) if c_sigma else ()) + ((("layer_norm", nm_a[1]),) if nm_a is not None else ())
    return obs_dim, act_dim, (tuple(ha), tuple(hc), act_a) + tags, "net"


def _attach_gauss_policy(algorithm, policy_forward: str, sampling: str, noise_seed) -> None:
    """the collector's `policy(batch)` / `policy.map_action(act)` (data/collector.py:735-744) on the engine's
    inference kernels -- `tianshou_amd.policy.attach` gives `algorithm.policy` a subclass of its own class whose forward reads
    the engine's device-resident parameters.  policy_forward="torch" keeps the reference's torch forward."""
    if policy_forward not in ("hip", "torch"):
        raise ValueError("policy_forward must be 'hip' or 'torch'")
    if policy_forward == "torch":
        return
    from . import policy as HP

    obs_dim, act_dim, hidden, kind = algorithm._hip_dims
    actor = algorithm.policy.actor
    ka, _ = _net_keys(actor, algorithm.critic)
    max_action = None if getattr(actor, "_unbounded", False) else float(actor.max_action)
    kw = dict(device=str(algorithm._hip_device), sampling=sampling, noise_seed=noise_seed, obs_dim=obs_dim, act_dim=act_dim,
              max_action=max_action, actor_keys=tuple(ka))
    if kind == "fused":
        HP.attach(algorithm.policy, "gauss", algorithm, **kw)
    elif kind == "wide":
        from . import npg as NG

        HP.attach(algorithm.policy, "gauss_wide", algorithm, hidden=int(hidden), n_actor=int(NG.layout(obs_dim, hidden, act_dim)["actor_count"]), **kw)
    elif "conditioned_sigma" not in hidden[3:]:              # "net" without conditioned sigma (that head keeps the torch forward)
        import ctypes as C

        from . import _lib

        ln_eps = _ln_eps_of(hidden)
        out = (C.c_int64 * 3)()
        desc = _lib.NetDesc.make(obs_dim, list(hidden[0]), hidden[2], _lib.NetDesc.LAYERNORM if ln_eps is not None else 0, ln_eps=ln_eps or 0.0)
        _lib.check(_lib.load().ts_net_layout(C.byref(desc), _lib.i64(act_dim), out))
        HP.attach(algorithm.policy, "gauss_net", algorithm, hidden=tuple(hidden[0]), activation=hidden[2], n_actor=int(out[1]),
                  ln_eps=ln_eps, **kw)


def make_hip_ppo(algo: str = "ppo", ref=None, base=None):
    """Returns the HipPPO class (imports tianshou lazily); algo="a2c": HipA2C(A2C), same networks.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`).  `base`: a subclass of the reference's PPO to build
    the same body over (make_hip_gail: GAIL)."""
    A2CTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.a2c", "A2CTrainingStats")
    SequenceSummaryStats = _ref(ref, "tianshou.data", "SequenceSummaryStats")
    Batch = _ref(ref, "tianshou.data", "Batch")
    PPO = _on_policy_base(algo, ref) if base is None else base

    from . import ppo_wide as PW

    class HipPPO(_HipGlue, PPO):
        def __init__(self, *args, device="cuda", permutations="device", perm_seed=None, data_parallel=False, group=None,
                     allreduce=None, shard_buffer=True, policy_forward="hip", sampling="device", noise_seed=None, **kwargs):
            """`data_parallel=True` (one process per GPU, torch.distributed initialised): `update()` mirrors only this
            rank's sub-buffers of `buffer` (`shard_buffer`, by env id; pass False when every rank collects into its own
            buffer), computes values / GAE / log pi_old shard-locally with GLOBAL return statistics, and every minibatch
            step all-reduces the flat gradient (`tianshou_amd.distributed.DataParallelPPO`); `allreduce`: None =
            torch.distributed (RCCL), "native" = the C-ABI exchange incl. the one-shot path for the 44 KB payload, or any
            in-place sum callable.  Replicas stay bit-identical.  `group`: the process group of the replicas.

            `permutations`: "device" (default) expands a private key (`perm_seed`, the update counter, the repeat and the
            rank) with ts_random_permutation on the GPU: a keyed bijection per repeat, statistically equivalent to
            Batch.split's shuffles, and NumPy's global generator -- which the collector shares -- is left untouched.
            `perm_seed=None` takes ONE draw from NumPy's global generator at construction, so that `np.random.seed` /
            `seed_everything` select the shuffle sequence as they do in the reference (pass an int to fix it); the seed and
            the update counter are saved with `hip_extra_state()` / restored with `load_hip_extra_state()` (a resumed run
            continues the sequence); `state_dict()` itself keeps the reference's format.
            "host" draws np.random.permutation(N) per repeat exactly like Batch.split (batch.py:1209): the reference's
            sequence for a given seed (the mode the parity tests use), at ~10 ms of host time per 2^20 entries -- 100 ms
            of a 12 ms update(), i.e. ~1.4 k instead of ~14 k update-steps/s at the C2 size.

            `policy_forward="hip"` (default): `self.policy` -- what the Collector calls once per vector step
            (collector.py:735-744) -- gets a subclass of its own class whose `forward` and `map_action` run on the engine's
            inference kernels and read its device-resident parameters (`tianshou_amd.policy`); "torch" keeps the reference's
            forward.  `sampling`: "device" draws dist.sample()'s noise with the engine's counter-based generator
            (`noise_seed`; torch's generator untouched), "torch" from torch's CPU generator in the reference's order."""
            super().__init__(*args, **kwargs)
            if permutations not in ("host", "device"):
                raise ValueError("permutations must be 'host' or 'device'")
            self._hip_perms = permutations
            if perm_seed is None:
                perm_seed = int(np.random.randint(0, 2**31 - 1)) if permutations == "device" else 0
            self._hip_perm_seed, self._hip_updates = int(perm_seed), 0
            self._hip_device = torch.device(device)
            self._hip_dims = _check_supported(self.policy.actor, self.critic)
            self._hip_dp_setup(data_parallel, group, allreduce, shard_buffer)
            self._hip_engine = None
            self._hip_glue_init()
            self._hip_batch = None
            self._hip_synced = False
            _attach_gauss_policy(self, policy_forward, sampling, noise_seed)

        # -- the shuffle key travels BESIDE the checkpoint ---------------------------------------------
        # state_dict() stays in the reference's format (a HipPPO checkpoint loads into the reference PPO / A2C class with
        # strict=True, nested in a parent module or not); the (seed, update counter) pair of the device permutations is
        # saved / restored explicitly, e.g. torch.save({"model": algo.state_dict(), "hip": algo.hip_extra_state()}, f).
        # The collector forward's sampling-noise counter (`sampling="device"`) travels with them.
        def hip_extra_state(self) -> dict:
            return {"perm_seed": int(self._hip_perm_seed), "updates": int(self._hip_updates), **_policy_extra_state(self)}

        def load_hip_extra_state(self, state: dict) -> None:
            self._hip_perm_seed, self._hip_updates = int(state["perm_seed"]), int(state["updates"])
            _load_policy_extra_state(self, state)
            self._hip_key_loaded = True

        def load_state_dict(self, state_dict, *args, **kwargs):
            # checkpoints of round-4 builds carried the pair inline -- under "_hip_perm_state", or "<prefix>_hip_perm_state"
            # when the algorithm was saved as a sub-module of a parent: taken out so that strict loading sees the reference's keys
            legacy = [k for k in state_dict if k == "_hip_perm_state" or k.endswith("._hip_perm_state")]
            if legacy:
                state_dict = dict(state_dict)
                for k in legacy:
                    st = state_dict.pop(k)
                    if k == "_hip_perm_state":
                        self._hip_perm_seed, self._hip_updates = int(st[0]), int(st[1])
            out = super().load_state_dict(state_dict, *args, **kwargs)
            if self.__dict__.get("_hip_key_loaded") is not True:          # (load_hip_extra_state() may come first)
                self._hip_key_loaded = "_hip_perm_state" in legacy        # (checked at the next update, see _update_with_batch)
            return out

        def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
            # the same legacy key when THIS module is loaded as part of a parent's state_dict (nn.Module.load_state_dict recurses
            # through _load_from_state_dict, not through load_state_dict)
            state_dict.pop(prefix + "_hip_perm_state", None)
            return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

        # -- engine life cycle ------------------------------------------------------------------
        def _hip_params(self):
            ka, kc = _net_keys(self.policy.actor, self.critic)      # == TIANSHOU_ACTOR_KEYS / _CRITIC_KEYS for Net[h, h]
            return params_by_keys(self.policy.actor, ka) + params_by_keys(self.critic, kc)

        def _hip_parts(self, eng=None):
            """One vector: the actor's tensors, then the critic's, in `_hip_params()` order (13 for Net[h, h])."""
            obs_dim, act_dim, hidden, kind = self._hip_dims
            params, dev = self._hip_params(), self._hip_device
            if kind == "fused":
                conv = (lambda t: torch.cat([x.detach().reshape(-1).float() for x in t]).to(dev).contiguous(),
                        lambda f: torch.split(f, [p.numel() for p in params]))
            elif kind == "net":
                ha, hc, kw = list(hidden[0]), list(hidden[1]), dict(layer_norm=_ln_eps_of(hidden) is not None)
                cs = "conditioned_sigma" in hidden[3:]
                na = (4 if kw["layer_norm"] else 2) * len(ha) + 2 + (2 if cs else 1)
                conv = (lambda t: torch.cat([PW.net_flat_from_tensors(list(t[:na]), obs_dim, ha, act_dim, dev, conditioned_sigma=cs, **kw),
                                             PW.net_flat_from_tensors(list(t[na:]), obs_dim, hc, None, dev, **kw)]).contiguous(),
                        lambda f: sum(eng.flat_to_tensors(f), []))
            else:
                conv = (lambda t: PW.flat_from_tensors(list(t[:7]), list(t[7:]), obs_dim, hidden, act_dim, dev),
                        lambda f: sum(PW.flat_to_tensors(f, obs_dim, hidden, act_dim), []))
            return [_OnPart("params", ("adam_m", "adam_v"), self.optim, params, *conv)]

        def _hip_build_engine(self):
            """A fresh engine from the torch parameters (`_engine` loads the optimizer state into it)."""
            obs_dim, act_dim, hidden, kind = self._hip_dims
            flat, cfg = self._hip_parts()[0].flat(), ppo_config_from(self)
            if kind == "fused":
                return PPOEngine(obs_dim, act_dim, flat, cfg)
            if kind == "net":
                ln_eps = _ln_eps_of(hidden)
                return PW.NetPPOEngine(obs_dim, act_dim, hidden[0], hidden[1], hidden[2], flat, cfg, layer_norm=ln_eps is not None,
                                       ln_eps=ln_eps or 1e-5, conditioned_sigma="conditioned_sigma" in hidden[3:])
            return PW.WidePPOEngine(obs_dim, act_dim, hidden, flat, cfg)

        def _engine(self):
            if self._hip_engine is None:
                self._hip_engine = _on_load(self, self._hip_build_engine())
            return self._hip_engine

        def _hip_rewards(self, eng, obs, act, rew):
            """The rewards the returns are computed from: the buffer's (HipGAIL: the discriminator's)."""
            return rew

        def _hip_runner(self, eng):
            if not self._hip_dp_on:
                return eng
            from .distributed import DataParallelPPO, DataParallelWidePPO

            return self._hip_dp(DataParallelPPO if self._hip_dims[3] == "fused" else DataParallelWidePPO, eng)

        def _hip_write_back(self) -> None:
            """After every update(): parameters (the collector acts with the torch modules) and ret_rms.  The Adam moments are
            only needed by `state_dict()` (algorithm_base.py:523-543) and move there (`_hip_flush`)."""
            _on_write_back(self, optimizer=False)
            self._hip_adam_dirty = True

        def _hip_flush(self) -> None:
            if getattr(self, "_hip_adam_dirty", False):
                _on_write_back(self, params=False)
                self._hip_adam_dirty = False

        # -- Algorithm.update ---------------------------------------------------------------------------
        def update(self, buffer, batch_size, repeat):
            """`OnPolicyAlgorithm.update` -> `Algorithm._update` (algorithm_base.py:586-631, 854-865), same steps in the
            same order, with `buffer.sample(0)` - a host fancy-index copy of every key, 1.4 s at 2^20 transitions -
            replaced by the device mirror of the buffer: only the slots written since the previous update cross PCIe,
            `sample_indices(0)`, the gathers and the unfinished-slot cuts run as kernels."""
            _require_gpu(self._hip_device, type(self).__name__)
            if not self.policy.is_within_training_step:
                raise RuntimeError(
                    f"update() was called outside of a training step as signalled by {self.policy.is_within_training_step=} "
                    "(see tianshou.utils.torch_utils.policy_within_training_step)")
            if buffer is None:
                return super().update(buffer, batch_size, repeat)
            import time

            start = time.time()
            m = _mirror(self, buffer, self._hip_device)
            self._hip_synced = True
            indices = m.sample_indices(0)
            batch = self._preprocess_batch(Batch(), buffer, indices)
            was_training = self.training                          # torch_train_mode (torch_utils.py:14-22)
            try:
                self.train(True)
                stat = self._update_with_batch(batch, batch_size, repeat)
            finally:
                self.train(was_training)
            if hasattr(buffer, "update_weight"):
                self._postprocess_batch(batch, buffer, m.to_global(indices).cpu().numpy())
            for lr_scheduler in self.lr_schedulers:
                lr_scheduler.step()
            stat.train_time = time.time() - start
            return stat

        # -- hooks ------------------------------------------------------------------------------------
        def _preprocess_batch(self, batch, buffer, indices):
            """a2c.py:239-247 / ppo.py:146-162.  Works on the device mirror at `indices` (the host copies in `batch`,
            when the caller is the reference's own `Algorithm._update`, are not read)."""
            from .returns import cut_positions

            _require_gpu(self._hip_device, type(self).__name__)
            eng = self._engine()
            if self._hip_synced:
                m, self._hip_synced = self._hip_mirror, False
            else:
                m = _mirror(self, buffer, self._hip_device)
            idx = indices if isinstance(indices, torch.Tensor) else \
                torch.as_tensor(np.asarray(indices, np.int64), device=self._hip_device)
            whole = idx.numel() == m.maxsize and m.indices_are_identity()     # sample(0) of full, unwrapped sub-buffers
            take = (lambda x: x) if whole else (lambda x: m.gather_tensor(x, idx))   # noqa: E731
            obs_next = take(m.obs_next) if m.obs_next is not None else m.gather_tensor(m.obs, m.next(idx))
            cut, d_n = cut_positions(m, idx)                                   # algorithm_base.py:715
            runner = self._hip_runner(eng)                                     # the engine, or its data-parallel wrapper
            obs, act = take(m.obs), take(m.act)
            b = runner.preprocess(obs, obs_next, act, self._hip_rewards(eng, obs, act, take(m.rew)), take(m.terminated),
                                  take(m.truncated), cut, d_n)
            self._hip_batch = b
            batch.v_s, batch.returns, batch.adv = b["v_s"], b["returns"], b["adv"]
            batch.act = b["act"]
            if algo == "ppo":                                                  # A2C has none (a2c.py:239-247)
                batch.logp_old = b["logp_old"]
            return batch

        def _update_with_batch(self, batch, batch_size, repeat):
            self._hip_refresh_lr()
            eng = self._engine()
            n = int(self._hip_batch["obs"].shape[0])
            if self._hip_perms == "host":
                perms = [np.random.permutation(n) for _ in range(repeat)]    # Batch.split, batch.py:1209
            else:
                from .buffer import random_permutation

                if self.__dict__.get("_hip_key_loaded") is False and eng.adam_step > 0:
                    # a trained checkpoint came in through load_state_dict alone: the optimizer continues, the shuffle key does not
                    import warnings

                    warnings.warn("HipPPO: resuming from a checkpoint without its device-permutation key: the shuffle sequence "
                                  "restarts from this object's own (perm_seed, 0).  Save `hip_extra_state()` beside `state_dict()` "
                                  "and restore it with `load_hip_extra_state()` to continue the sequence.", stacklevel=2)
                self.__dict__["_hip_key_loaded"] = None
                self._hip_updates += 1
                rank = self._hip_world()[0]
                key = ((self._hip_perm_seed * 0x9E3779B97F4A7C15) ^ (self._hip_updates << 20) ^ (rank << 52)) & (2**64 - 1)
                perms = [random_permutation(n, key + r, self._hip_device) for r in range(repeat)]
            losses, steps = self._hip_runner(eng).update(self._hip_batch, batch_size, repeat, perms)
            stats = _a2c_stats(A2CTrainingStats, SequenceSummaryStats.from_sequence, losses, steps)
            eng.check()                                                # surfaces a stuck GAE hand-off (never observed)
            self._hip_write_back()
            return stats

    if algo == "a2c":
        HipPPO.__name__ = HipPPO.__qualname__ = "HipA2C"
    return HipPPO


# ---------------------------------------------------------------------------------------------------
# GAIL (imitation/gail.py): HipPPO over the reference's GAIL, plus the discriminator engine (tianshou_amd/gail.py)
# ---------------------------------------------------------------------------------------------------
_GAIL_KEY = 0xA5A5A5A55A5A5A5A          # sub-key of (perm_seed, update counter) for the discriminator's draws


def make_hip_gail(ref=None):
    """Returns HipGAIL(GAIL): HipPPO's body over the reference's GAIL (gail.py:30-248) -- every keyword, engine kind and the
    device buffer mirror are HipPPO's -- with the discriminator on the engine: `_preprocess_batch` replaces the rewards by
    -logsigmoid(-D(obs, act)) (ts_gail_reward on the mirror's rows, float32, before the discriminator is updated);
    `_update_with_batch` first runs all discriminator steps in one call (ts_gail_disc_steps), then HipPPO's update, and returns
    GailTrainingStats from one read of the per-step statistics.
    Discriminator: ContinuousCritic(preprocess_net=Net(..., concat=True)) or any Linear / tanh / ReLU chain with one output
    (no normalisation layers), Adam or RMSprop.  The expert buffer's obs / act are copied to the device when the engine is built
    (`hip_invalidate()` after changing the expert buffer).
    Randomness follows `permutations=`: "host" makes the reference's draws in its order -- np.random.permutation(N) for the split,
    `expert_buffer.sample_indices(bsz)` once per step, then the PPO permutations; "device" uses the keyed device generators with
    sub-keys of (perm_seed, update counter) and touches neither NumPy's nor the expert buffer's generator.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    GAIL = _ref(ref, "tianshou.algorithm.imitation.gail", "GAIL")
    GailTrainingStats = _ref(ref, "tianshou.algorithm.imitation.gail", "GailTrainingStats")
    SequenceSummaryStats = _ref(ref, "tianshou.data", "SequenceSummaryStats")
    HipPPO = make_hip_ppo("ppo", ref, base=GAIL)

    from . import gail as GA
    from .ppo_wide import net_flat_to_tensors

    class HipGAIL(HipPPO):
        def __init__(self, *args, data_parallel=False, disc_route="auto", **kwargs):
            if data_parallel:
                raise NotImplementedError("HipGAIL: data_parallel=True is not supported (the discriminator steps are not all-reduced)")
            policy = kwargs.get("policy", args[0] if args else None)
            space = getattr(policy, "action_space", None)
            if space is not None and (hasattr(space, "n") or hasattr(space, "nvec")):
                raise NotImplementedError(f"HipGAIL: continuous actions only (found a {type(space).__name__} action space; the "
                                          "reference's cat([obs, act], dim=1) needs action vectors)")
            super().__init__(*args, **kwargs)
            obs_dim, act_dim = self._hip_dims[0], self._hip_dims[1]
            # raises NotImplementedError naming what was found (layer norm, another layer class, an output size != 1)
            self._hip_disc = GA.describe_module(self.disc_net, obs_dim + act_dim)[:2]
            if disc_route not in GA.ROUTES:
                raise ValueError(f"disc_route must be one of {sorted(GA.ROUTES)}")
            self._hip_disc_route = disc_route
            optimizer_fields(self.disc_optim._optim)                       # (raises on an optimizer the engine does not implement)
            self._hip_gail_rew = None

        # -- engine life cycle: the discriminator is a second part, owned by `eng.gail` ------------------------------------------
        def _hip_disc_config(self):
            of = optimizer_fields(self.disc_optim._optim)
            return GA.GAILConfig(disc_update_num=int(self.disc_update_num), optimizer=of["optimizer"], lr=of["lr"],
                                 betas=tuple(of.get("betas", (0.9, 0.999))), eps=of["adam_eps"], weight_decay=of["weight_decay"],
                                 rms_alpha=of.get("rms_alpha", 0.99), rms_momentum=of.get("rms_momentum", 0.0),
                                 rms_centered=of.get("rms_centered", False), max_grad_norm=self.disc_optim._max_grad_norm,
                                 route=self._hip_disc_route)

        def _hip_parts(self, eng=None):
            obs_dim, act_dim = self._hip_dims[0], self._hip_dims[1]
            hidden, _ = self._hip_disc
            params, dev = GA.describe_module(self.disc_net, obs_dim + act_dim)[2], self._hip_device
            return super()._hip_parts(eng) + [
                _OnPart("disc", ("state_m", "state_v"), self.disc_optim, params,
                        lambda t: GA.GAILDiscriminator.flat_from_tensors(t, obs_dim, act_dim, hidden, dev),
                        lambda f: net_flat_to_tensors(f, obs_dim + act_dim, hidden, 1, False), holder="gail", step="optim_step")]

        def _hip_build_engine(self):
            eng = super()._hip_build_engine()
            obs_dim, act_dim = self._hip_dims[0], self._hip_dims[1]
            hidden, activation = self._hip_disc
            eb = self.expert_buffer
            eng.gail = GA.GAILDiscriminator(obs_dim, act_dim, hidden, activation, self._hip_parts()[-1].flat(),
                                            np.asarray(eb.obs, dtype=np.float32), np.asarray(eb.act, dtype=np.float32),
                                            self._hip_disc_config())
            return eng

        def _hip_refresh_lr(self) -> None:
            super()._hip_refresh_lr()
            eng = self._hip_engine
            if eng is not None:
                opt = self.disc_optim._optim
                lr = float(opt.param_groups[0]["lr"])
                if any(float(g["lr"]) != lr for g in opt.param_groups):
                    raise NotImplementedError("the HIP engines take one learning rate per optimizer")
                eng.gail.cfg.lr = lr
                eng.gail.cfg.disc_update_num = int(self.disc_update_num)
                opt._opt_called = True

        def _hip_expert_layout(self, dev):
            """(offset, lengths) of the expert buffer's sub-buffers on the device, for the seeded index sampler."""
            eb = self.expert_buffer
            if hasattr(eb, "_lengths"):
                off, ln = np.asarray(eb._offset, np.int64), np.asarray(eb._lengths, np.int64)
            else:
                off, ln = np.zeros(1, np.int64), np.asarray([len(eb)], np.int64)
            return torch.as_tensor(off, device=dev), torch.as_tensor(ln, device=dev)

        # -- hooks ----------------------------------------------------------------------------------------------------------------
        def _hip_rewards(self, eng, obs, act, rew):
            """gail.py:203-206, with the parameters the discriminator has BEFORE this update's steps."""
            self._hip_gail_rew = eng.gail.reward(obs, act)
            return self._hip_gail_rew

        def _preprocess_batch(self, batch, buffer, indices):
            batch = super()._preprocess_batch(batch, buffer, indices)
            batch.rew = self._hip_gail_rew
            return batch

        def _update_with_batch(self, batch, batch_size, repeat):
            self._hip_refresh_lr()
            eng = self._engine()
            b, dev = self._hip_batch, self._hip_device
            n = int(b["obs"].shape[0])
            bsz, steps = GA.chunking(n, self.disc_update_num)        # ValueError before anything is launched (gail.py:224: bsz 0)
            if self._hip_perms == "host":
                perm = np.random.permutation(n)                       # Batch.split, batch.py:1209
                ei = np.concatenate([np.asarray(self.expert_buffer.sample_indices(bsz), np.int64) for _ in range(steps)])
            else:
                import ctypes as C

                from . import _lib
                from .buffer import random_permutation

                u = self._hip_updates + 1                             # the update counter HipPPO's permutations take below
                key = ((self._hip_perm_seed * 0x9E3779B97F4A7C15) ^ (u << 20) ^ _GAIL_KEY) & (2**64 - 1)
                perm = random_permutation(n, key, dev)
                off, ln = self._hip_expert_layout(dev)
                ei = torch.empty(steps * bsz, dtype=torch.int64, device=dev)
                err = torch.zeros(1, dtype=torch.int32, device=dev)
                for k in range(steps):                                # (the sampler's output is grouped by sub-buffer: one draw per step)
                    _lib.check(_lib.load().ts_sample_indices_seeded(
                        _lib.ptr(off), _lib.i64(off.numel()), _lib.ptr(ln), C.c_uint64(key), C.c_uint64(k), _lib.i64(bsz),
                        C.c_void_p(ei.data_ptr() + 8 * k * bsz), _lib.ptr(err), _lib.current_stream(dev)))
            dstats = eng.gail.disc_update(b["obs"], b["act"], perm, ei)
            stat = super()._update_with_batch(batch, batch_size, repeat)
            arr = dstats.cpu().numpy().astype(np.float64)             # the one read of the discriminator's statistics
            seq = SequenceSummaryStats.from_sequence
            return GailTrainingStats(**stat.__dict__, disc_loss=seq(arr[:, 0]), acc_pi=seq(arr[:, 1]), acc_exp=seq(arr[:, 2]))

    return HipGAIL


# ---------------------------------------------------------------------------------------------------
# NPG (npg.py) / TRPO (trpo.py) on the MuJoCo actor-critic
# ---------------------------------------------------------------------------------------------------
def _make_hip_natural(algo: str, ref=None):
    SequenceSummaryStats = _ref(ref, "tianshou.data", "SequenceSummaryStats")

    from . import npg as NG

    if algo == "npg":
        Base = _ref(ref, "tianshou.algorithm.modelfree.npg", "NPG")
        Stats = _ref(ref, "tianshou.algorithm.modelfree.npg", "NPGTrainingStats")
    else:
        Base = _ref(ref, "tianshou.algorithm.modelfree.trpo", "TRPO")
        Stats = _ref(ref, "tianshou.algorithm.modelfree.trpo", "TRPOTrainingStats")
    who = "HipNPG" if algo == "npg" else "HipTRPO"

    class HipNatural(_HipGlue, Base):
        def __init__(self, *args, device="cuda", **kwargs):
            """Net[h1, h2] tanh actor and critic (the nets of examples/mujoco/mujoco_npg.py, any two widths): the fused / GEMM
            passes of NPGEngine.  Every other `Net(hidden_sizes=[...], activation=Tanh | ReLU | None)` trunk -- other depths,
            ReLU, actor and critic trunks that differ -- (round 6): NetNPGEngine, layer by layer on the GEMM kernels."""
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            actor, critic = self.policy.actor, self.critic
            sa, sc = actor.state_dict(), critic.state_dict()
            if getattr(actor, "_c_sigma", True) or not getattr(actor, "_unbounded", False):
                raise NotImplementedError(f"{who}: actor must be unbounded with a state-independent sigma_param")
            _, ha, act_a = _trunk_spec(actor, "actor")               # (raises for anything but Linear + Tanh / ReLU / nothing)
            _, hc, act_c = _trunk_spec(critic, "critic")
            ka, kc = _net_keys(actor, critic)                        # == TIANSHOU_ACTOR_KEYS / _CRITIC_KEYS for two hidden layers
            if set(sa.keys()) != set(ka) or list(sc.keys()) != list(kc) or act_a != act_c:
                raise NotImplementedError(f"{who}: actor and critic must be Net trunks with one activation + a linear mu / value head "
                                          "(examples/mujoco/mujoco_npg.py)")
            self._hip_akeys, self._hip_ckeys = ka, kc
            self._hip_two = len(ha) == 2 and len(hc) == 2 and act_a == "tanh"
            if not 1 <= int(sa["mu.model.0.weight"].shape[0]) <= 32:
                raise NotImplementedError(f"{who}: at most 32 actions")
            if self._hip_two:
                from . import widths as WD

                try:        # any two hidden widths per network (round 6): embedded by zero padding (tianshou_amd.widths)
                    la, lc = [sa[k] for k in ka[:6]], [sc[k] for k in kc]
                    self._hip_sizes = {"actor": WD.two_layer_widths(la), "critic": WD.two_layer_widths(lc)}
                    self._hip_hidden = WD.common_hidden(la, lc)
                except NotImplementedError as e:
                    raise NotImplementedError(f"{who}: hidden layers of widths up to 1024 per network ({e})") from None
            else:
                if max(ha + hc) > 1024 or not 1 <= len(ha) <= 7 or not 1 <= len(hc) <= 7:
                    raise NotImplementedError(f"{who}: 1 .. 7 hidden layers of widths up to 1024 per network")
                self._hip_trunks = (list(ha), list(hc), act_a)
            _adam_of(self.optim)
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_parts(self, eng=None):
            """The actor (no optimizer: natural-gradient steps) and the critic; the per-layer engine brings its own converters."""
            dev = self._hip_device
            aparams = params_by_keys(self.policy.actor, self._hip_akeys)
            cparams = params_by_keys(self.critic, self._hip_ckeys)
            obs_dim, act_dim = aparams[0].shape[1], aparams[-3].shape[0]          # (the actor ends in mu.weight, mu.bias, sigma_param)
            if self._hip_two:
                hidden, sizes = self._hip_hidden, self._hip_sizes     # (two widths per network, embedded: tianshou_amd.widths)
                conv = (lambda t: NG.actor_flat_from_torch(t, obs_dim, hidden, act_dim, dev),
                        lambda f: NG.actor_flat_to_torch(f, obs_dim, hidden, act_dim, sizes=sizes["actor"]),
                        lambda t: NG.critic_flat_from_torch(t, obs_dim, hidden, dev),
                        lambda f: NG.critic_flat_to_torch(f, obs_dim, hidden, sizes=sizes["critic"]))
            elif eng is not None:
                conv = (eng.actor_from_tensors, eng.actor_to_tensors, eng.critic_from_tensors, eng.critic_to_tensors)
            else:
                from .ppo_wide import net_flat_from_tensors as nf

                ha, hc, _ = self._hip_trunks
                conv = (lambda t: nf(t, obs_dim, ha, act_dim, dev), None, lambda t: nf(t, obs_dim, hc, None, dev), None)
            return [_OnPart("actor", None, None, aparams, conv[0], conv[1]),
                    _OnPart("critic", ("critic_m", "critic_v"), self.optim, cparams, conv[2], conv[3])]

        def _engine(self):
            if self._hip_engine is None:
                actor, critic = self._hip_parts()
                obs_dim, act_dim = actor.params[0].shape[1], actor.params[-3].shape[0]
                _, g = _adam_of(self.optim)
                cfg = NG.NPGConfig(algo=algo, gamma=self.gamma, gae_lambda=self.gae_lambda,
                                   optim_critic_iters=self.optim_critic_iters,
                                   trust_region_size=float(getattr(self, "trust_region_size", 0.5)),
                                   advantage_normalization=self.advantage_normalization, return_scaling=self.return_scaling,
                                   damping=float(self._damping), max_kl=float(getattr(self, "max_kl", 0.01)),
                                   backtrack_coeff=float(getattr(self, "backtrack_coeff", 0.8)),
                                   max_backtracks=int(getattr(self, "max_backtracks", 10)), lr=g["lr"], betas=tuple(g["betas"]),
                                   adam_eps=g["eps"], max_grad_norm=self.optim._max_grad_norm)
                Engine, net = (NG.NPGEngine, (self._hip_hidden,)) if self._hip_two else (NG.NetNPGEngine, self._hip_trunks)
                self._hip_engine = _on_load(self, Engine(obs_dim, act_dim, *net, actor.flat(), critic.flat(), cfg))
            return self._hip_engine

        _hip_write_back = _on_write_back

        def _preprocess_batch(self, batch, buffer, indices):
            eng, t, cut = _on_host_batch(self, who, buffer, indices)
            b = self._hip_pre = eng.preprocess(t(batch.obs, torch.float32), t(batch.obs_next, torch.float32),
                                               t(batch.act, torch.float32), t(batch.rew, torch.float64), t(batch.terminated),
                                               t(batch.truncated), cut)
            batch.v_s, batch.returns, batch.adv, batch.logp_old, batch.act = b["v_s"], b["returns"], b["adv"], b["logp_old"], b["act"]
            return batch

        def _update_with_batch(self, batch, batch_size, repeat):
            self._hip_refresh_lr()
            eng = self._hip_engine
            perms = [np.random.permutation(len(batch)) for _ in range(repeat)]     # Batch.split, batch.py:1209
            stats, _ = eng.update(self._hip_pre, batch_size, repeat, perms)
            arr = stats.cpu().numpy().astype(np.float64)                          # one D2H per update()
            self._hip_write_back()
            seq = SequenceSummaryStats.from_sequence
            kw = dict(actor_loss=seq(arr[:, 0]), vf_loss=seq(arr[:, 1]), kl=seq(arr[:, 2]))
            if algo == "trpo":
                kw["step_size"] = seq(arr[:, 3])
            return Stats(**kw)

    HipNatural.__name__ = HipNatural.__qualname__ = who
    return HipNatural


def make_hip_npg(ref=None):
    """Returns HipNPG(NPG): `_preprocess_batch` / `_update_with_batch` (npg.py:123-193) on the engine.  Supported nets:
    examples/mujoco/mujoco_npg.py:103-128 (Net[h, h] tanh actor and critic, unbounded Gaussian actor with sigma_param).
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    return _make_hip_natural("npg", ref)


def make_hip_trpo(ref=None):
    """Returns HipTRPO(TRPO): the same hooks with TRPO's step size and line search (trpo.py:123-214)."""
    return _make_hip_natural("trpo", ref)


def make_hip_reinforce(ref=None):
    """Returns HipReinforce(Reinforce): `_preprocess_batch` / `_update_with_batch` (reinforce.py:346-382) on the engine.
    Supported net: the actor of examples/mujoco/mujoco_reinforce.py:84-103 (Net[h, h] tanh, unbounded Gaussian, sigma_param).
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    LossSequenceTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "LossSequenceTrainingStats")
    Reinforce = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "Reinforce")
    SequenceSummaryStats = _ref(ref, "tianshou.data", "SequenceSummaryStats")

    from . import npg as NG
    from . import ppo_wide as PW
    from . import reinforce as RF

    who = "HipReinforce"

    class HipReinforce(_HipGlue, Reinforce):
        def __init__(self, *args, device="cuda", **kwargs):
            """Net[h, h] tanh (h a multiple of 32) under an unbounded actor with plain Adam -- the nets of
            examples/mujoco/mujoco_reinforce.py -- runs on the fused step kernel / the Net[h, h] GEMM path as before; every
            other `Net(hidden_sizes=[...], activation=Tanh | ReLU | None)` trunk, the reference's default bounded actor
            (max_action * tanh), Adam with weight decay and RMSprop (optim.py:89-140) take the per-layer engine
            (`reinforce.NetReinforceEngine`, round 6), and so do `Net(norm_layer=nn.LayerNorm)` trunks (common.py:25-39).
            conditioned_sigma and other norm layers raise."""
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            actor = self.policy.actor
            sa = actor.state_dict()
            if getattr(actor, "_c_sigma", True):
                raise NotImplementedError(f"{who}: the actor needs a state-independent sigma_param (no conditioned sigma)")
            stems, hidden_sizes, act_name = _trunk_spec(actor, "actor", norm=True)   # (raises for anything but Linear + Tanh / ReLU)
            nm = _trunk_norm(actor, "actor")                                         # MLP(norm_layer=nn.LayerNorm): per-layer engine
            trunk_keys = ([f"{st}.{x}" for st in stems for x in ("weight", "bias")] if nm is None else
                          [f"{x}.{y}" for a, b in zip(stems, nm[0]) for x in (a, b) for y in ("weight", "bias")])
            self._hip_keys = trunk_keys + ["mu.model.0.weight", "mu.model.0.bias", "sigma_param"]
            if set(sa.keys()) != set(self._hip_keys) or sa["mu.model.0.weight"].shape[1] != hidden_sizes[-1]:
                raise NotImplementedError(f"{who}: the actor must be ContinuousActorProbabilistic over a Net trunk with a single-Linear mu head")
            of = optimizer_fields(self.optim._optim)
            bounded = not getattr(actor, "_unbounded", False)
            plain = of["optimizer"] == "adam" and not of["weight_decay"]
            legacy = (nm is None and act_name == "tanh" and len(hidden_sizes) == 2 and hidden_sizes[0] == hidden_sizes[1]
                      and hidden_sizes[0] % 32 == 0 and not bounded and plain and self._hip_keys == list(TIANSHOU_ACTOR_KEYS))
            if not legacy and (len(hidden_sizes) > 7 or max(hidden_sizes) > 1024 or sa["mu.model.0.weight"].shape[0] > 32):
                raise NotImplementedError(f"{who}: trunks of up to 7 hidden layers of at most 1024 units, at most 32 actions")
            self._hip_kind = "legacy" if legacy else "net"
            self._hip_net = (hidden_sizes, act_name, float(actor.max_action) if bounded else None, of)
            self._hip_ln = None if nm is None else float(nm[1])
            self._hip_engine = None
            self._hip_glue_init()

        def _dims(self):
            sa = self.policy.actor.state_dict()
            hidden, obs_dim = sa[self._hip_keys[0]].shape
            return obs_dim, hidden, sa["mu.model.0.weight"].shape[0]

        def _hip_parts(self, eng=None):
            params = params_by_keys(self.policy.actor, self._hip_keys)
            (hidden, obs_dim), act_dim = params[0].shape, params[-3].shape[0]     # (`_dims()` without its walk; the keys end in mu, sigma_param)
            dev, sizes, ln = self._hip_device, list(self._hip_net[0]), self._hip_ln is not None
            if self._hip_kind == "legacy":
                conv = (lambda t: NG.actor_flat_from_torch(t, obs_dim, hidden, act_dim, dev),
                        lambda f: NG.actor_flat_to_torch(f, obs_dim, hidden, act_dim))
            else:
                conv = (lambda t: PW.net_flat_from_tensors(list(t), obs_dim, sizes, act_dim, dev, layer_norm=ln),
                        lambda f: PW.net_flat_to_tensors(f, obs_dim, sizes, act_dim, True, layer_norm=ln))
            return [_OnPart("actor", ("adam_m", "adam_v"), self.optim, params, *conv)]

        def _engine(self):
            if self._hip_engine is None:
                part, = self._hip_parts()
                obs_dim, hidden, act_dim = self._dims()
                of = self._hip_net[3]
                drc = self.discounted_return_computation
                cfg = RF.ReinforceConfig(gamma=drc.gamma, return_standardization=drc.return_standardization, lr=of["lr"],
                                         betas=tuple(of.get("betas", (0.9, 0.999))), adam_eps=of["adam_eps"],
                                         max_grad_norm=self.optim._max_grad_norm)
                if self._hip_kind == "legacy":
                    eng = RF.ReinforceEngine(obs_dim, act_dim, hidden, part.flat(), cfg)
                else:
                    hidden_sizes, act_name, max_action, _ = self._hip_net
                    eng = RF.NetReinforceEngine(obs_dim, act_dim, hidden_sizes, act_name, part.flat(), cfg, max_action=max_action,
                                                optimizer=of, layer_norm=self._hip_ln is not None, ln_eps=self._hip_ln or 1e-5)
                self._hip_engine = _on_load(self, eng)
            return self._hip_engine

        _hip_write_back = _on_write_back

        def _preprocess_batch(self, batch, buffer, indices):
            eng, t, cut = _on_host_batch(self, who, buffer, indices)
            batch.returns = eng.preprocess(t(batch.rew, torch.float64), t(batch.terminated), t(batch.truncated), cut)
            self._hip_obs, self._hip_act = t(batch.obs, torch.float32), t(batch.act, torch.float32)
            _on_ret_rms(self, eng)                       # (the return statistics move here already, not only after the update)
            return batch

        def _update_with_batch(self, batch, batch_size, repeat):
            self._hip_refresh_lr()
            eng = self._hip_engine
            perms = [np.random.permutation(len(batch)) for _ in range(repeat)]     # Batch.split, batch.py:1209
            losses, _ = eng.update(self._hip_obs, self._hip_act, batch.returns, batch_size, repeat, perms)
            arr = losses.cpu().numpy().astype(np.float64).reshape(-1)              # one D2H per update()
            self._hip_write_back()
            return LossSequenceTrainingStats(loss=SequenceSummaryStats.from_sequence(arr))

    return HipReinforce


def make_hip_a2c():
    """HipA2C(A2C) on the MuJoCo actor-critic of HipPPO (a2c.py:249-290 = the fused step kernel's algo 1)."""
    return make_hip_ppo("a2c")


def make_hip_a2c_discrete():
    """HipA2CDiscrete(A2C) on the shared-trunk MLP of HipPPODiscrete."""
    return make_hip_ppo_discrete("a2c")


def make_hip_a2c_cnn():
    """HipA2CCnn(A2C) on the Atari actor-critic of HipPPOCnn."""
    return make_hip_ppo_cnn("a2c")


# ---------------------------------------------------------------------------------------------------
# DQN (dqn.py:288-404) on DQNet
# ---------------------------------------------------------------------------------------------------
def _require_gpu(device: torch.device, who: str) -> None:
    if device.type != "cuda":
        raise RuntimeError(f"{who} needs an MI355X (device='cuda'); there is no CPU fallback")


def _adam_of(optim):
    opt = optim._optim
    g = opt.param_groups[0]
    if type(opt).__name__ != "Adam" or g.get("weight_decay", 0) != 0 or g.get("amsgrad", False):
        raise NotImplementedError("the HIP engines support torch.optim.Adam without weight decay / amsgrad")
    return opt, g


def _mirror(algorithm, buffer, device):
    """Device mirror of the host replay buffer, refreshed incrementally on every update()."""
    from .buffer import DeviceReplayBuffer

    m = getattr(algorithm, "_hip_mirror", None)
    if m is None or algorithm._hip_mirror_src is not buffer:
        shard = algorithm._hip_shard_range(buffer) if hasattr(algorithm, "_hip_shard_range") else None
        m = DeviceReplayBuffer.from_tianshou(buffer, device=device, env_range=shard)
        algorithm._hip_mirror, algorithm._hip_mirror_src = m, buffer
    else:
        m.sync_from_tianshou(buffer)
    return m


# -- what the Q-learning classes (HipDQN, HipDRQN, HipQRDQN / HipC51 / HipDiscreteCQL, HipIQN, HipRainbow) share: one path for
# the torch state into a fresh engine (`_q_load`) and one back (`_q_write_back`), both reading the same `_QState` --------------
class _QState(NamedTuple):
    """How a Q network's torch state maps to its engine's flat vectors.  Every class builds its own in `_hip_qstate()`, per
    call: the converters are looked up in their engine module when they are used, not when the class is made."""
    keys: list            # names of the parameters, in the order the converters take and return them
    from_torch: Callable  # the engine module's flat_from_torch(tensors, *dims, device)
    to_torch: Callable    # the engine module's flat_to_torch(flat, *dims)
    dims: Callable        # engine -> the dims tuple of the two converters


def _q_layout(buffer, who: str):
    """-> (c, h, w, stack_num) of a frame buffer: whole [c, h, w] observations, or single frames stacked c times."""
    obs = np.asarray(buffer.obs)
    stack = int(getattr(buffer, "stack_num", 1))
    if stack > 1:
        if obs.ndim != 3:
            raise NotImplementedError(f"{who}: frame stacking needs single [h, w] frames per slot")
        return stack, obs.shape[1], obs.shape[2], stack
    if obs.ndim != 4:
        raise NotImplementedError(f"{who}: observations must be [c, h, w]")
    return obs.shape[1], obs.shape[2], obs.shape[3], 1


def _q_begin(algo, who: str, batch, buffer, indices):
    """Every `_preprocess_batch`, once the buffer's layout is accepted: -> (device mirror of `buffer`, `indices` as a device tensor, kept in `_hip_idx` for
    `_update_with_batch`); a prioritized buffer's importance weights move to the device."""
    _require_gpu(algo._hip_device, who)
    m = _mirror(algo, buffer, algo._hip_device)
    idx = algo._hip_idx = torch.as_tensor(np.asarray(indices, np.int64), device=algo._hip_device)
    if hasattr(batch, "weight"):
        batch.weight = torch.as_tensor(np.asarray(batch.weight), dtype=torch.float32, device=algo._hip_device)
    return m, idx


def _q_config_fields(algo) -> dict:
    """The target / optimizer fields every Q engine's config has."""
    _, g = _adam_of(algo.optim)
    return dict(gamma=algo.gamma, n_step=algo.n_step, target_update_freq=algo.target_update_freq, lr=g["lr"],
                betas=tuple(g["betas"]), adam_eps=g["eps"], max_grad_norm=algo.optim._max_grad_norm)


def _q_flat(algo, dims: tuple) -> torch.Tensor:
    """The online network's parameters as the flat vector an engine is constructed from."""
    st = algo._hip_qstate()
    return st.from_torch([p.detach() for p in params_by_keys(algo.policy.model, st.keys)], *dims, algo._hip_device)


def _q_old_params(algo, st: _QState):
    """The lagged network's parameters; `model_old` is the bare module or its EvalModeModuleWrapper."""
    return params_by_keys(getattr(algo.model_old, "module", algo.model_old), st.keys)


def _q_load(algo, eng):
    """Torch state -> a fresh engine (built from `_q_flat`): update counter, Adam moments (resume from a checkpoint), lagged
    network.  The inverse of `_q_write_back`.  -> eng"""
    st, dev = algo._hip_qstate(), algo._hip_device
    dims = st.dims(eng)
    eng.iter = algo._iter
    ms, vs, eng.adam_step = adam_state(algo.optim._optim, params_by_keys(algo.policy.model, st.keys))
    eng.adam_m, eng.adam_v = st.from_torch(ms, *dims, dev), st.from_torch(vs, *dims, dev)
    if eng.params_old is not None:
        eng.params_old = st.from_torch([p.detach() for p in _q_old_params(algo, st)], *dims, dev)
    return eng


def _q_write_back(algo) -> None:
    """`_hip_write_back` of the Q-learning classes: engine parameters, lagged parameters and Adam state -> the torch modules
    and torch.optim, every parameter through `_hip_put` (which leaves out what somebody else has written)."""
    eng = algo.__dict__.get("_hip_engine_obj")
    if eng is None:
        return
    st = algo._hip_qstate()
    dims = st.dims(eng)
    params = params_by_keys(algo.policy.model, st.keys)
    with torch.no_grad():
        for p, t in zip(params, st.to_torch(eng.params, *dims)):
            algo._hip_put(p, t)
        if eng.params_old is not None:
            for p, t in zip(_q_old_params(algo, st), st.to_torch(eng.params_old, *dims)):
                algo._hip_put(p, t)
    store_adam_state(algo.optim._optim, params, st.to_torch(eng.adam_m, *dims), st.to_torch(eng.adam_v, *dims), eng.adam_step)


# -- what the off-policy actor-critic classes (HipSAC, HipREDQ, HipDiscreteSAC, HipTD3 / HipDDPG / HipTD3BC) share: the same two
# paths over one `_ACPart` per network (`_ac_load`, `_ac_write_back`), the constructor envelope, the config fields, the preamble --
class _ACPart(NamedTuple):
    """How one network's torch state maps to its engine's flat vectors `eng.<name>`, `eng.<name>_old`, `eng.<name>_m` / `_v`.
    Every class body builds its parts in `_hip_parts()`, per call (the converters are looked up in their engine module when they
    are used) and closes them over its dims, so the engine modules' differing converter signatures end there."""
    name: str             # the engine attribute stem
    module: object        # the online torch module
    old: object           # the lagged torch module, or None
    optim: object         # the Algorithm.Optimizer wrapper of `module`
    keys: list            # names of the parameters, in the order the converters take and return them
    from_torch: Callable  # tensors in `keys` order (parameters or Adam moments) -> flat
    to_torch: Callable    # flat -> tensors in `keys` order
    step: str             # the engine counter that is this optimizer's step count at write-back
    load_step: bool       # whether torch.optim's step is loaded into that counter (else the body sets it from the algorithm)

    def flat(self) -> torch.Tensor:
        """The online network's parameters as the flat vector an engine is constructed from."""
        return self.from_torch([p.detach() for p in params_by_keys(self.module, self.keys)])


def _ac_nets(algo, who: str, envelope: str, nets, optims, widths=None) -> dict:
    """The constructor envelope.  `nets`: (name, module, depth -> state_dict keys) per network, actor first: one depth for all of
    them (`_hip_depth`), one activation (`_hip_actfn`), the hidden widths (`_hip_sizes`; `widths[name]`: tensors -> widths of a
    network that is no plain MLP) embedded in one engine width (`_hip_hidden`), Adam on every optimizer, and the actor's
    `_hip_obs_dim` / `_hip_act_dim`.  -> {name: keys}"""
    from . import widths as WD

    keys, depth = {}, None
    for name, mod, keys_of in nets:
        have = list(mod.state_dict().keys())
        d = next((d for d in range(1, WD.MAX_DEPTH + 1) if have == keys_of(d)), None)
        if d is None or depth not in (None, d):
            raise NotImplementedError(f"{who}: {envelope}")
        depth, keys[name] = d, have
    algo._hip_depth = depth
    algo._hip_actfn = _trunk_activation([mod for _, mod, _ in nets], who)
    try:        # any hidden widths per network: embedded by zero padding into the engine's Net[h] * depth (tianshou_amd.widths)
        sizes = {}
        for name, mod, _ in nets:
            t = [p.detach() for p in params_by_keys(mod, keys[name])]
            sizes[name] = widths[name](t) if name in (widths or {}) else WD.layer_widths(t, len(t) // 2 - depth)
        algo._hip_sizes, algo._hip_hidden = sizes, WD.engine_hidden(sizes.values())
    except NotImplementedError as e:
        raise NotImplementedError(f"{who}: hidden layers of widths up to 1024 per network ({e})") from None
    for o in optims:
        _adam_of(o)
    first = dict(nets[0][1].named_parameters())
    algo._hip_obs_dim = int(first[keys[nets[0][0]][0]].shape[1])
    algo._hip_act_dim = int(first[keys[nets[0][0]][2 * depth]].shape[0])
    return keys


def _ac_config_fields(algo) -> dict:
    """The target / optimizer fields every actor-critic engine's config has."""
    ga, gc = _adam_of(algo.policy_optim)[1], _adam_of(algo.critic_optim)[1]
    return dict(gamma=algo.gamma, tau=algo.tau, n_step=algo.n_step_return_horizon, actor_lr=ga["lr"], critic_lr=gc["lr"],
                betas=tuple(ga["betas"]), adam_eps=ga["eps"])


def _ac_entropy_fields(algo, AutoAlpha) -> dict:
    """The entropy-coefficient fields of SACConfig / REDQConfig: a fixed alpha, or AutoAlpha's (sac.py:175-210)."""
    auto = isinstance(algo.alpha, AutoAlpha)
    return dict(alpha=0.0 if auto else float(algo.alpha.value), auto_alpha=auto,
                target_entropy=float(algo.alpha._target_entropy) if auto else 0.0,
                log_alpha0=float(algo.alpha._log_alpha.item()) if auto else 0.0,
                alpha_lr=algo.alpha._optim.param_groups[0]["lr"] if auto else 0.0)


def _ac_begin(algo, who: str, buffer, indices):
    """Every `_preprocess_batch`: -> (engine, device mirror of `buffer`, `indices` as a device tensor, kept in `_hip_idx` for
    `_update_with_batch`)."""
    _require_gpu(algo._hip_device, who)
    eng = algo._engine()
    m = _mirror(algo, buffer, algo._hip_device)
    idx = algo._hip_idx = torch.as_tensor(np.asarray(indices, np.int64), device=algo._hip_device)
    return eng, m, idx


def _ac_load(algo, eng):
    """Torch state -> a fresh engine (built from every part's `flat()`): lagged networks, Adam moments and step counts (resume from
    a checkpoint), log alpha's moments.  The inverse of `_ac_write_back`.  -> eng"""
    for part in algo._hip_parts():
        if part.old is not None:
            setattr(eng, part.name + "_old", part.from_torch([p.detach() for p in params_by_keys(part.old, part.keys)]))
        ms, vs, step = adam_state(part.optim._optim, params_by_keys(part.module, part.keys))
        setattr(eng, part.name + "_m", part.from_torch(ms))
        setattr(eng, part.name + "_v", part.from_torch(vs))
        if part.load_step:
            setattr(eng, part.step, max(getattr(eng, part.step), step))
    if getattr(eng.cfg, "auto_alpha", False):
        st = algo.alpha._optim.state.get(algo.alpha._log_alpha, {})
        if "exp_avg" in st:
            eng.log_alpha_m[0], eng.log_alpha_v[0] = float(st["exp_avg"]), float(st["exp_avg_sq"])
    return eng


def _ac_write_back(algo) -> None:
    """`_hip_write_back` of the actor-critic classes: engine parameters, lagged parameters, log alpha and Adam state -> the torch
    modules and torch.optim, every parameter through `_hip_put` (which leaves out what somebody else has written).  An optimizer
    that has not stepped yet (REDQ's delayed actor) gets no state; log alpha's optimizer steps with the actor's."""
    eng = algo.__dict__.get("_hip_engine_obj")
    if eng is None:
        return
    parts, put = algo._hip_parts(), algo._hip_put
    # the parameter lists, looked up once per engine (`params_by_keys` walks the module tree: six walks per TD3 write-back)
    cache = algo.__dict__.get("_hip_ac_params")
    if cache is None or cache[0] is not eng:
        cache = algo.__dict__["_hip_ac_params"] = (eng, [(params_by_keys(part.module, part.keys),
                                                            () if part.old is None else params_by_keys(part.old, part.keys)) for part in parts])
    with torch.no_grad():
        for part, (params, old) in zip(parts, cache[1]):
            for p, t in zip(params, part.to_torch(getattr(eng, part.name))):
                put(p, t)
            if part.old is not None:
                for p, t in zip(old, part.to_torch(getattr(eng, part.name + "_old"))):
                    put(p, t)
            step = getattr(eng, part.step)
            if step:
                store_adam_state(part.optim._optim, params, part.to_torch(getattr(eng, part.name + "_m")),
                                 part.to_torch(getattr(eng, part.name + "_v")), step)
        if getattr(eng.cfg, "auto_alpha", False):
            put(algo.alpha._log_alpha, eng.log_alpha[0])
            step = getattr(eng, parts[0].step)
            if step:
                store_adam_state(algo.alpha._optim, [algo.alpha._log_alpha], [eng.log_alpha_m[0]], [eng.log_alpha_v[0]], step)


# -- what the on-policy classes (HipPPO / HipA2C, HipNPG / HipTRPO, HipReinforce, HipPPOCnn / HipA2CCnn, HipPPODiscrete / HipA2CDiscrete)
# share: the same two paths over one `_OnPart` per flat engine vector (`_on_load`, `_on_write_back`), the statistics, the host preamble --
class _OnPart(NamedTuple):
    """How one flat engine vector `eng.<name>` and its two optimizer-state vectors map to torch parameters.  Every class body
    builds its parts in `_hip_parts(eng)`, per call (the converters are looked up in their engine module when they are used) and
    closes them over its dims; `eng` is None before the engine exists, when only `flat()` is asked for."""
    name: str             # the engine attribute that holds the parameters: "params", "actor" or "critic"
    moments: tuple | None  # the engine attributes of the two moment vectors; None: no optimizer (the NPG / TRPO actor)
    optim: object         # the Algorithm.Optimizer wrapper of `params` (None with `moments`)
    params: list          # the torch parameters in converter order; one part may span modules (PPO: the actor's, then the critic's)
    from_torch: Callable  # tensors in `params` order (parameters or moments) -> flat
    to_torch: Callable    # flat -> tensors in `params` order
    holder: str | None = None   # the engine attribute of the sub-engine that owns the vectors (HipGAIL's discriminator); None: the engine
    step: str = "adam_step"     # the owner's attribute with the optimizer's step count

    def own(self, eng):
        return eng if self.holder is None else getattr(eng, self.holder)

    def flat(self) -> torch.Tensor:
        """The parameters as the flat vector an engine is constructed from."""
        return self.from_torch([p.detach() for p in self.params])


def _on_ret_rms(algo, eng=None):
    """The running return statistics' holder: the algorithm's own (a2c.py, npg.py) or REINFORCE's return computation
    (reinforce.py:249-271); with `eng`, the engine's three scalars are first stored there."""
    rms = getattr(getattr(algo, "discounted_return_computation", algo), "ret_rms", None)   # None: a wrapper without returns (HipICM)
    if eng is not None and rms is not None:
        rms.mean, rms.var, rms.count = eng.ret_rms
    return rms


def _on_load(algo, eng):
    """Torch state -> a fresh engine (built from every part's `flat()`): optimizer moments and step count (resume from a
    checkpoint, algorithm_base.py:523-543), return statistics.  The inverse of `_on_write_back`.  -> eng"""
    for part in algo._hip_parts(eng):
        if part.moments is not None:
            own = part.own(eng)
            ms, vs, step = adam_state(part.optim._optim, part.params)
            setattr(own, part.step, step)
            setattr(own, part.moments[0], part.from_torch(ms))
            setattr(own, part.moments[1], part.from_torch(vs))
    rms = _on_ret_rms(algo)
    if rms is not None:
        eng.ret_rms = [float(rms.mean), float(rms.var), float(rms.count)]
    return eng


def _on_write_back(algo, params: bool = True, optimizer: bool = True) -> None:
    """`_hip_write_back` of the on-policy classes.  `params`: engine parameters -> the torch modules, every parameter through
    `_hip_put` (which leaves out what somebody else has written; device-to-device when the modules live on the GPU), and the three
    return statistics.  `optimizer`: moments and step count -> torch.optim (HipPPO defers them to `_hip_flush`)."""
    eng = algo.__dict__.get("_hip_engine_obj")
    if eng is None:
        return
    with torch.no_grad():
        for part in algo._hip_parts(eng):
            own = part.own(eng)
            if params:
                for p, t in zip(part.params, part.to_torch(getattr(own, part.name))):
                    algo._hip_put(p, t)
            if optimizer and part.moments is not None:
                m, v = (part.to_torch(getattr(own, name)) for name in part.moments)
                store_adam_state(part.optim._optim, part.params, m, v, getattr(own, part.step))
    if params:
        _on_ret_rms(algo, eng)


def _a2c_stats(Stats, seq, losses, steps):
    """[steps, 4+] per-step (loss, actor loss, value loss, entropy loss) on the device -> A2CTrainingStats; one D2H per update()."""
    arr = losses.cpu().numpy().astype(np.float64)
    return Stats(loss=seq(arr[:, 0]), actor_loss=seq(arr[:, 1]), vf_loss=seq(arr[:, 2]), ent_loss=seq(arr[:, 3]), gradient_steps=steps)


def _on_host_batch(algo, who: str, buffer, indices):
    """`_preprocess_batch` of the classes that read the host batch (HipNPG / HipTRPO, HipReinforce): -> (engine, host array ->
    device tensor[, cast], the positions in `indices` of the unfinished slots (algorithm_base.py:715) on the device)."""
    _require_gpu(algo._hip_device, who)
    eng, dev = algo._engine(), algo._hip_device

    def t(x, dt=None):
        x = torch.as_tensor(np.ascontiguousarray(x), device=dev)
        return x if dt is None else x.to(dt)

    return eng, t, t(np.nonzero(np.isin(indices, buffer.unfinished_index()))[0])


def _dqn_config(algo):
    from . import dqn as D

    return D.DQNConfig(is_double=algo.is_double, huber_delta=algo.huber_loss_delta, **_q_config_fields(algo))


def _dqn_update(algo, batch, Stats):
    """`_update_with_batch` of HipDRQN, and of HipDQN where the two hooks are two library calls: `_preprocess_batch` left the
    batch's observations in `_hip_obs` and the returns on the batch."""
    eng, m = algo._hip_engine, algo._hip_mirror
    weight = batch.pop("weight", None)
    # (index-only sampling: the batch carries no host copy of the actions; the mirror's rows are the same values)
    act = torch.as_tensor(np.asarray(batch.act), device=algo._hip_device) if hasattr(batch, "act") else m.act[algo._hip_idx]
    runner = eng
    if algo._hip_dp_on:
        from .distributed import DataParallelDQN

        runner = algo._hip_dp(DataParallelDQN, eng)
    loss, td = runner.update_with_batch(algo._hip_obs, act, batch.returns.reshape(-1), weight)
    algo._iter = eng.iter
    batch.weight = td                                                         # prio-buffer, dqn.py:401
    algo._hip_after_update()                                                  # write-back now ("eager") or when read ("lazy")
    return Stats(loss=float(loss.item()))


def make_hip_dqn(ref=None):
    """Returns HipDQN(DQN): `_preprocess_batch` / `_update_with_batch` (dqn.py:257-275, 381-404) on the engine.
    Supported model: DQNet(c, h, w, n_act) (atari_network.py:60-122), Adam; buffer either stores whole [c, h, w]
    observations or single frames with stack_num = c (save_only_last_obs); obs_next optional.
    What the engine learnt reaches the torch modules and torch.optim in `_q_write_back`, which is `_hip_write_back` of this
    class and of the other Q-learning classes below; `_HipGlue._hip_after_update` decides when.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    DQN = _ref(ref, "tianshou.algorithm.modelfree.dqn", "DQN")
    SimpleLossTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "SimpleLossTrainingStats")
    Batch = _ref(ref, "tianshou.data", "Batch")

    from . import dqn as D

    class HipDQN(_HipGlue, DQN):
        def __init__(self, *args, device="cuda", data_parallel=False, group=None, allreduce=None, policy_forward="hip",
                     write_back="auto", host_batch=False, **kwargs):
            """`data_parallel=True`: one process per GPU, every rank samples its own minibatch from its own buffer (its
            envs) and `_update_with_batch` all-reduces the flat gradient + loss (`DataParallelDQN`); PER priorities stay
            rank-local.  `allreduce`: None = torch.distributed, "native" = the C-ABI RCCL exchange, or a callable.
            `policy_forward="hip"`: `DiscreteQLearningPolicy.forward` (dqn.py:101-143), which the Collector
            calls per vector step, runs on `ts_dqn_forward` with the engine's parameters (`tianshou_amd.policy`); the
            epsilon-greedy `add_exploration_noise` stays the reference's.
            Hook-level throughput (as HipSAC's): `host_batch=False` lets `update()` sample indices only -- the hooks read frames,
            actions and rewards from the device mirror by index, the host copy `buffer.sample()` makes of the batch (two stacked
            observations per transition: 29 MB for 512 Atari transitions) is never looked at (True: the reference's own
            `Algorithm._update`); `write_back="auto"` keeps the updates in the engine until somebody reads the torch modules (lazy
            whenever the policy forward is the engine's; "eager" = the two networks and the optimizer state after every update,
            27 MB of device copies in ~40 torch ops; `hip_sync()` forces it)."""
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            self._hip_host_batch = bool(host_batch)
            sd = self.policy.model.state_dict()
            if list(sd.keys()) != D.TIANSHOU_KEYS:
                raise NotImplementedError("HipDQN: the model must be DQNet(c, h, w, action_shape) without extra layers")
            _adam_of(self.optim)
            self._hip_engine = None
            self._hip_glue_init()
            self._hip_dp_setup(data_parallel, group, allreduce, shard_buffer=False)
            if policy_forward not in ("hip", "torch"):
                raise ValueError("policy_forward must be 'hip' or 'torch'")
            if policy_forward == "hip":
                from . import policy as HP

                HP.attach(self.policy, "q", self, device=str(self._hip_device), n_act=int(sd[D.TIANSHOU_KEYS[-1]].numel()))
            self._hip_set_write_back(write_back, attached=policy_forward == "hip")

        def update(self, buffer, sample_size):
            if self._hip_host_batch or buffer is None:
                return super().update(buffer, sample_size)
            return self._hip_offpolicy_update(buffer, sample_size, Batch)

        def _hip_qstate(self):
            return _QState(D.TIANSHOU_KEYS, D.flat_from_torch, D.flat_to_torch, lambda eng: (eng.c, eng.h, eng.w, eng.n_act))

        def _engine(self, c, h, w):
            if self._hip_engine is None:
                n_act = self.policy.model.state_dict()[D.TIANSHOU_KEYS[-1]].numel()
                eng = D.DQNEngine(c, h, w, n_act, _q_flat(self, (c, h, w, n_act)), _dqn_config(self))
                self._hip_engine = _q_load(self, eng)
            return self._hip_engine

        def _preprocess_batch(self, batch, buffer, indices):
            c, h, w, stack = self._layout(buffer, "HipDQN")
            m, idx = _q_begin(self, "HipDQN", batch, buffer, indices)
            eng = self._engine(c, h, w)
            # Inside HipDQN.update()'s own sequence (`_hip_offpolicy_update`: nobody reads the batch between the two hooks) on the
            # Atari layout (single uint8 frames, stack 4, no stored obs_next) the two hooks are ONE library call, made by
            # `_update_with_batch` (ts_dqn_learn_rows; `batch.returns` is attached there).  Called on its own (the reference's
            # `_update`, `host_batch=True`, data parallel, other layouts) the hook computes the returns here.
            self.__dict__["_hip_deferred"] = (self.__dict__.get("_hip_own_sequence", False) and not self._hip_dp_on and stack == c
                                              and hasattr(eng, "rows_ok") and eng.rows_ok(m, m.obs, m.act)
                                              and not os.environ.get("TS_DQN_TWO_CALLS"))
            if self.__dict__["_hip_deferred"]:
                return batch
            nxt = m.obs_next if m.obs_next is not None else None
            # the batch's own observations, gathered here so that Q_online(batch.obs) of _update_with_batch can run beside the
            # two obs_next passes of _target_q (DQNEngine.prefetch_forward); data-parallel runs keep the plain order
            # (on a frame buffer without obs_next, one launch gathers both stacked observations: DQNEngine.preprocess_with_obs)
            self._hip_obs, ret = eng.preprocess_with_obs(m, m.obs, idx, stack, obs_next_frames=nxt,
                                                         prefetch=not self._hip_dp_on)
            batch.returns = ret.reshape(-1, 1)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            if not self.__dict__.pop("_hip_deferred", False):
                return _dqn_update(self, batch, SimpleLossTrainingStats)
            eng, m = self._hip_engine, self._hip_mirror
            loss, td, ret = eng.learn_rows(m, m.obs, m.act, self._hip_idx, batch.pop("weight", None))
            batch.returns = ret.reshape(-1, 1)
            self._iter = eng.iter
            batch.weight = td                                                 # prio-buffer, dqn.py:401
            self._hip_after_update()
            return SimpleLossTrainingStats(loss=float(loss.item()))

        _layout = staticmethod(_q_layout)
        _hip_write_back = _q_write_back

    return HipDQN


# ---------------------------------------------------------------------------------------------------
# DQN on the Recurrent Q network (DRQN, test/discrete/test_drqn.py)
# ---------------------------------------------------------------------------------------------------
def make_hip_drqn(ref=None):
    """Returns HipDRQN(DQN): the DQN hooks (dqn.py:257-275, 381-404) on the engine for a Recurrent model
    (utils/net/common.py:372-452) over a buffer with stack_num (the LSTM's sequence length) and vector observations.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    DQN = _ref(ref, "tianshou.algorithm.modelfree.dqn", "DQN")
    SimpleLossTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "SimpleLossTrainingStats")

    from . import drqn as R

    class HipDRQN(_HipGlue, DQN):
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            sd = self.policy.model.state_dict()
            layers = sum(1 for k in sd if k.startswith("nn.weight_ih_l"))
            if layers < 1 or list(sd.keys()) != R.state_dict_keys(layers):
                raise NotImplementedError("HipDRQN: the model must be Recurrent(layer_num, state_shape, action_shape, hidden)")
            hidden, obs_dim = sd["fc1.weight"].shape
            n_act = sd["fc2.weight"].shape[0]
            if hidden % 32 or not 32 <= hidden <= 1024 or layers > 8 or n_act > 32:
                raise NotImplementedError("HipDRQN: hidden a multiple of 32 in [32, 1024], at most 8 layers and 32 actions")
            self._hip_dims = (obs_dim, hidden, layers, n_act)
            _adam_of(self.optim)
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_qstate(self):
            dims = self._hip_dims                 # (obs_dim, hidden, layers, n_act): what the engine was built with
            return _QState(R.state_dict_keys(dims[2]), R.flat_from_torch, R.flat_to_torch, lambda eng: dims)

        def _engine(self):
            if self._hip_engine is None:
                dims = self._hip_dims
                self._hip_engine = _q_load(self, R.RecurrentDQNEngine(*dims, _q_flat(self, dims), _dqn_config(self)))
            return self._hip_engine

        def _preprocess_batch(self, batch, buffer, indices):
            obs = np.asarray(buffer.obs)
            if obs.ndim != 2 or obs.shape[1] != self._hip_dims[0]:
                raise NotImplementedError("HipDRQN: the buffer must hold vector observations of the model's state_shape")
            m, idx = _q_begin(self, "HipDRQN", batch, buffer, indices)
            eng = self._engine()
            stack = int(getattr(buffer, "stack_num", 1))
            nxt = m.obs_next if m.obs_next is not None else None
            # the batch's own stacked observations are gathered here, so that their forward pass (the one _update_with_batch needs)
            # can run on a side stream beside the two obs_next passes of _target_q; data-parallel runs keep the plain order
            self._hip_obs, ret = eng.preprocess_with_obs(m, m.obs, idx, stack, obs_next_rows=nxt, prefetch=not self._hip_dp_on)
            batch.returns = ret.reshape(-1, 1)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            return _dqn_update(self, batch, SimpleLossTrainingStats)

        _hip_write_back = _q_write_back

    return HipDRQN


# ---------------------------------------------------------------------------------------------------
# QRDQN (qrdqn.py) / C51 (c51.py) on QRDQNet / C51Net
# ---------------------------------------------------------------------------------------------------
def _make_hip_distq(kind: str, ref=None, cql: bool = False):
    """`cql`: DiscreteCQL (imitation/discrete_cql.py), QRDQN with the conservative term -- the same hooks over
    tianshou_amd.dcql.DiscreteCQLEngine, with `min_q_weight` and the three-number statistics."""
    from . import distq as Q
    from . import dqn as D

    SimpleLossTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "SimpleLossTrainingStats")
    LossSequenceTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "LossSequenceTrainingStats")
    if kind == Q.QR:
        Base = _ref(ref, "tianshou.algorithm.modelfree.qrdqn", "QRDQN")
    else:
        Base = _ref(ref, "tianshou.algorithm.modelfree.c51", "C51")
    who = "HipQRDQN" if kind == Q.QR else "HipC51"
    if cql:
        from . import dcql as CQ

        Base = _ref(ref, "tianshou.algorithm.imitation.discrete_cql", "DiscreteCQL")
        DiscreteCQLTrainingStats = _ref(ref, "tianshou.algorithm.imitation.discrete_cql", "DiscreteCQLTrainingStats")
        who = "HipDiscreteCQL"

    class HipDistQ(_HipGlue, Base):
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            if list(self.policy.model.state_dict().keys()) != D.TIANSHOU_KEYS:
                raise NotImplementedError(f"{who}: the model must be QRDQNet / C51Net (DQNet without extra layers)")
            _adam_of(self.optim)
            self._hip_engine = None
            self._hip_glue_init()

        def _n_atoms(self) -> int:
            return int(self.num_quantiles if kind == Q.QR else self.policy.num_atoms)

        def _hip_qstate(self):
            return _QState(D.TIANSHOU_KEYS, Q.flat_from_torch, Q.flat_to_torch,
                           lambda eng: (eng.c, eng.h, eng.w, eng.n_act, eng.cfg.n_atoms))

        def _engine(self, c, h, w):
            if self._hip_engine is None:
                n_atoms = self._n_atoms()
                n_out = self.policy.model.state_dict()[D.TIANSHOU_KEYS[-1]].numel()
                if n_out % n_atoms:
                    raise NotImplementedError(f"{who}: head width {n_out} is not a multiple of {n_atoms} atoms")
                n_act = n_out // n_atoms
                fields = dict(kind=kind, n_atoms=n_atoms, v_min=float(getattr(self.policy, "v_min", -10.0)),
                              v_max=float(getattr(self.policy, "v_max", 10.0)), **_q_config_fields(self))
                flat = _q_flat(self, (c, h, w, n_act, n_atoms))
                if cql:
                    cfg = CQ.DiscreteCQLConfig(min_q_weight=float(self.min_q_weight), **fields)
                    eng = CQ.DiscreteCQLEngine(c, h, w, n_act, flat, cfg)
                else:
                    eng = Q.DistQEngine(c, h, w, n_act, flat, Q.DistQConfig(**fields))
                self._hip_engine = _q_load(self, eng)
            return self._hip_engine

        def _preprocess_batch(self, batch, buffer, indices):
            c, h, w, self._hip_stack = self._layout(buffer, who)
            m, idx = _q_begin(self, who, batch, buffer, indices)
            eng = self._engine(c, h, w)
            batch.returns = eng.preprocess(m, m.obs, idx, self._hip_stack, obs_next_frames=m.obs_next)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            eng, m = self._hip_engine, self._hip_mirror
            idx, stack = self._hip_idx, self._hip_stack
            weight = batch.pop("weight", None)
            obs = D.gather_obs_nhwc(m.obs, m, idx, stack, as_u8=True)
            obs_next = None
            if kind == Q.C51:                     # batch.obs_next = buffer[indices].obs_next (buffer_base.py:624-626)
                if m.obs_next is not None:
                    obs_next = D.gather_obs_nhwc(m.obs_next, m, idx, stack, as_u8=True)
                else:
                    obs_next = D.gather_obs_nhwc(m.obs, m, m.next(idx), stack, as_u8=True)
            act = torch.as_tensor(np.asarray(batch.act), device=self._hip_device)
            if cql:
                eng.cfg.min_q_weight = float(self.min_q_weight)                   # read at every update, as the learning rate
            loss, prio = eng.update_with_batch(obs, act, batch.returns, weight, obs_next_nhwc=obs_next)
            self._iter = eng.iter
            batch.weight = prio                                                   # prio-buffer, qrdqn.py:128 / c51.py:157
            self._hip_after_update()
            if cql:
                total, qr_loss, cql_loss = loss.tolist()                          # one transfer for the three numbers
                return DiscreteCQLTrainingStats(loss=total, qr_loss=qr_loss, cql_loss=cql_loss)       # discrete_cql.py:109-113
            if kind == Q.QR:
                return SimpleLossTrainingStats(loss=float(loss.item()))
            return LossSequenceTrainingStats(loss=float(loss.item()))            # as c51.py:160

        _layout = staticmethod(_q_layout)
        _hip_write_back = _q_write_back

    HipDistQ.__name__ = HipDistQ.__qualname__ = who
    return HipDistQ


def make_hip_qrdqn(ref=None):
    """Returns HipQRDQN(QRDQN): `_preprocess_batch` / `_update_with_batch` (dqn.py:257-275, qrdqn.py:93-131) on the
    engine.  Supported model: QRDQNet (atari_network.py:211-235), Adam; buffer layouts as HipDQN.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    return _make_hip_distq("qr", ref)


def make_hip_c51(ref=None):
    """Returns HipC51(C51): `_preprocess_batch` / `_update_with_batch` (dqn.py:257-275, c51.py:120-160) on the engine.
    Supported model: C51Net (atari_network.py:125-151) with C51Policy's support, Adam; buffer layouts as HipDQN.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    return _make_hip_distq("c51", ref)


def make_hip_discrete_cql(ref=None):
    """Returns HipDiscreteCQL(DiscreteCQL): `_preprocess_batch` / `_update_with_batch` (dqn.py:257-275 with qrdqn.py:93-104,
    imitation/discrete_cql.py:80-113) on the engine (tianshou_amd/dcql.py).  Supported model: QRDQNet, Adam; buffer layouts as
    HipDQN -- the offline case is a plain ReplayBuffer / VectorReplayBuffer without `weight`, a prioritized buffer works as well.
    `min_q_weight` is read from the algorithm at every update; the statistics are DiscreteCQLTrainingStats(loss, qr_loss,
    cql_loss).  `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    return _make_hip_distq("qr", ref, cql=True)


def make_hip_iqn(ref=None):
    """Returns HipIQN(IQN): `_preprocess_batch` / `_update_with_batch` (dqn.py:257-275 with qrdqn.py:94-106, iqn.py:156-183) on
    the engine (tianshou_amd/iqn.py).  Supported model: ImplicitQuantileNetwork(preprocess_net=DQNet(features_only=True),
    hidden_sizes=[512], num_cosines=64) as examples/atari/atari_iqn.py builds it, Adam; buffer layouts as HipDQN.  The sample
    sizes come from the policy (`online_sample_size`, `target_sample_size`).  The collector's `policy.forward` stays on torch.
    `hip_taus`: a callable, or an iterator, that yields the fraction tensors [B, N] in the reference's call order (target pass:
    online net, then lagged net if there is one; update pass: online net) -- a seeded reference run is replayed by passing
    its draws; without it the engine draws from its own stream (`hip_seed`, counter saved by `hip_extra_state()`).
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    from . import dqn as D
    from . import iqn as I

    SimpleLossTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "SimpleLossTrainingStats")
    Base = _ref(ref, "tianshou.algorithm.modelfree.iqn", "IQN")
    supported = ("HipIQN: the model must be ImplicitQuantileNetwork(preprocess_net=DQNet(features_only=True), "
                 "hidden_sizes=[512], num_cosines=64)")

    class HipIQN(_HipGlue, Base):
        def __init__(self, *args, device="cuda", hip_taus=None, hip_seed=0, **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            self._hip_check_model()
            _adam_of(self.optim)
            self._hip_taus = hip_taus
            self._hip_seed = int(hip_seed)
            self._hip_tau_counter = 0
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_check_model(self) -> None:
            sd = self.policy.model.state_dict()
            if list(sd.keys()) != I.TIANSHOU_KEYS:
                raise NotImplementedError(f"{supported}; got parameters {list(sd.keys())}")
            shapes = [tuple(sd[k].shape) for k in I.TIANSHOU_KEYS]
            convs_ok = (len(shapes[0]) == 4 and shapes[0][0] == 32 and shapes[0][2:] == (8, 8) and shapes[2] == (64, 32, 4, 4)
                        and shapes[4] == (64, 64, 3, 3))
            if not convs_ok:
                raise NotImplementedError(f"{supported}; the preprocess_net is not the DQNet convolution trunk")
            if shapes[6][0] != I.HIDDEN or shapes[8][1] != I.HIDDEN:
                raise NotImplementedError(f"{supported}; got hidden width {shapes[6][0]}")
            if shapes[10][1] != 64:
                raise NotImplementedError(f"{supported}; got num_cosines = {shapes[10][1]}")
            if not 1 <= shapes[8][0] <= 64:
                raise NotImplementedError("HipIQN: 1 <= number of actions <= 64")
            for name in ("online_sample_size", "target_sample_size"):
                if not 2 <= int(getattr(self.policy, name)) <= 64:
                    raise NotImplementedError(f"HipIQN: 2 <= policy.{name} <= 64")

        # -- the fraction counter travels BESIDE the checkpoint (state_dict() stays in the reference's format) ----------
        def hip_extra_state(self) -> dict:
            eng = self.__dict__.get("_hip_engine_obj")
            return {"tau_seed": int(self._hip_seed), "tau_counter": int(eng.tau_counter if eng is not None else self._hip_tau_counter)}

        def load_hip_extra_state(self, state: dict) -> None:
            self._hip_seed, self._hip_tau_counter = int(state["tau_seed"]), int(state["tau_counter"])
            eng = self.__dict__.get("_hip_engine_obj")
            if eng is not None:
                eng.cfg.seed, eng.tau_counter = self._hip_seed, self._hip_tau_counter

        def _hip_next_tau(self):
            src = self._hip_taus
            if src is None:
                return None
            t = src() if callable(src) else next(src)
            return torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t, dtype=torch.float32,
                                   device=self._hip_device)

        def _hip_qstate(self):
            return _QState(I.TIANSHOU_KEYS, I.flat_from_torch, I.flat_to_torch,
                           lambda eng: (eng.c, eng.h, eng.w, eng.n_act, eng.cfg.n_cos))

        def _engine(self, c, h, w):
            if self._hip_engine is None:
                n_act = int(self.policy.model.state_dict()[I.TIANSHOU_KEYS[8]].shape[0])
                cfg = I.IQNConfig(n_cos=64, sample_size=min(max(int(self.policy.sample_size), 2), 64),
                                  online_sample_size=int(self.policy.online_sample_size),
                                  target_sample_size=int(self.policy.target_sample_size), seed=self._hip_seed,
                                  **_q_config_fields(self))
                eng = I.IQNEngine(c, h, w, n_act, _q_flat(self, (c, h, w, n_act, 64)), cfg)
                eng.tau_counter = self._hip_tau_counter
                self._hip_engine = _q_load(self, eng)
            return self._hip_engine

        def _preprocess_batch(self, batch, buffer, indices):
            c, h, w, self._hip_stack = self._layout(buffer, "HipIQN")
            m, idx = _q_begin(self, "HipIQN", batch, buffer, indices)
            eng = self._engine(c, h, w)
            tau_online = self._hip_next_tau()                                    # qrdqn.py:100 / :103
            tau_target = self._hip_next_tau() if eng.params_old is not None else None      # qrdqn.py:101
            batch.returns = eng.preprocess(m, m.obs, idx, self._hip_stack, obs_next_frames=m.obs_next, tau_online=tau_online,
                                           tau_target=tau_target)
            self._hip_tau_counter = eng.tau_counter
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            eng, m = self._hip_engine, self._hip_mirror
            weight = batch.pop("weight", None)
            obs = D.gather_obs_nhwc(m.obs, m, self._hip_idx, self._hip_stack, as_u8=True)
            act = torch.as_tensor(np.asarray(batch.act), device=self._hip_device)
            loss, prio = eng.update_with_batch(obs, act, batch.returns, weight, tau=self._hip_next_tau())      # iqn.py:162
            self._iter = eng.iter
            self._hip_tau_counter = eng.tau_counter
            batch.weight = prio                                                   # prio-buffer, iqn.py:180
            self._hip_after_update()
            return SimpleLossTrainingStats(loss=float(loss.item()))

        _layout = staticmethod(_q_layout)
        _hip_write_back = _q_write_back

    return HipIQN


def make_hip_discrete_bcq(ref=None):
    """Returns HipDiscreteBCQ(DiscreteBCQ): `_preprocess_batch` / `_update_with_batch` (imitation/discrete_bcq.py:213-261) on
    the engine (tianshou_amd/bcq.py).  Supported model: policy.model and policy.imitator = DiscreteActor(preprocess_net,
    hidden_sizes=[512], softmax_output=False) on ONE shared DQNet(features_only=True), as examples/offline/atari_bcq.py builds
    them, with one Adam over the policy; buffer layouts as HipDQN -- a plain ReplayBuffer / VectorReplayBuffer; a prioritized
    one is accepted and its weights are ignored, as the reference ignores them.  The threshold (`policy._log_tau`) and
    `_weight_reg` are read from the algorithm at every update; the statistics are DiscreteBCQTrainingStats(loss, q_loss, i_loss,
    reg_loss).  The parameter root is the POLICY (fourteen parameters, the shared trunk once); `model_old` holds the first ten.
    The collector's `policy.forward` stays on torch.  `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    from . import bcq as BQ
    from . import dqn as D

    Base = _ref(ref, "tianshou.algorithm.imitation.discrete_bcq", "DiscreteBCQ")
    DiscreteBCQTrainingStats = _ref(ref, "tianshou.algorithm.imitation.discrete_bcq", "DiscreteBCQTrainingStats")
    supported = ("HipDiscreteBCQ: policy.model and policy.imitator must be DiscreteActor(preprocess_net, hidden_sizes=[512], "
                 "softmax_output=False) on one shared DQNet(features_only=True)")
    old_keys = [k[len("model."):] for k in BQ.TIANSHOU_KEYS[:BQ.N_LAGGED]]

    class HipDiscreteBCQ(_HipGlue, Base):
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            self._hip_check_model()
            _adam_of(self.optim)
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_check_model(self) -> None:
            pol = self.policy
            named = dict(pol.named_parameters())
            if list(named.keys()) != BQ.TIANSHOU_KEYS:
                raise NotImplementedError(f"{supported}; got parameters {list(named.keys())}")
            if getattr(pol.model, "preprocess", None) is not getattr(pol.imitator, "preprocess", None):
                raise NotImplementedError(f"{supported}; the two heads do not share one trunk object")
            shapes = [tuple(named[k].shape) for k in BQ.TIANSHOU_KEYS]
            convs_ok = (len(shapes[0]) == 4 and shapes[0][0] == 32 and shapes[0][2:] == (8, 8) and shapes[2] == (64, 32, 4, 4)
                        and shapes[4] == (64, 64, 3, 3))
            if not convs_ok:
                raise NotImplementedError(f"{supported}; the preprocess_net is not the DQNet convolution trunk")
            for j in (6, 10):
                if shapes[j][0] != BQ.HIDDEN or shapes[j + 2][1] != BQ.HIDDEN:
                    raise NotImplementedError(f"{supported}; got hidden width {shapes[j][0]}")
            if shapes[8][0] != shapes[12][0] or not 1 <= shapes[8][0] <= 64:
                raise NotImplementedError("HipDiscreteBCQ: both heads need the same number of actions, 1 <= n_act <= 64")
            if getattr(pol.model, "softmax_output", False) or getattr(pol.imitator, "softmax_output", False):
                raise NotImplementedError(f"{supported}; got softmax_output=True")
            if not self.freq > 0:
                raise NotImplementedError("HipDiscreteBCQ: BCQ needs target_update_freq > 0")
            opt_params = [p for g in self.optim._optim.param_groups for p in g["params"]]
            if len(self.optim._optim.param_groups) != 1 or {id(p) for p in opt_params} != {id(p) for p in named.values()}:
                raise NotImplementedError("HipDiscreteBCQ: one optimizer group over the policy's fourteen parameters")

        def _hip_old_params(self):
            """The lagged network's ten parameters; `model_old` is the bare module or its EvalModeModuleWrapper."""
            return params_by_keys(getattr(self.model_old, "module", self.model_old), old_keys)

        def _hip_read_scalars(self, eng) -> None:
            eng.cfg.log_tau = float(self.policy._log_tau)                         # read at every call, as the learning rate
            eng.cfg.imitation_logits_penalty = float(self._weight_reg)

        def _engine(self, c, h, w):
            if self._hip_engine is None:
                dev = self._hip_device
                params = params_by_keys(self.policy, BQ.TIANSHOU_KEYS)
                n_act = int(params[8].shape[0])
                dims = (c, h, w, n_act)
                _, g = _adam_of(self.optim)
                cfg = BQ.BCQConfig(gamma=self.gamma, n_step=self.n_step, target_update_freq=self.freq, lr=g["lr"],
                                   betas=tuple(g["betas"]), adam_eps=g["eps"], max_grad_norm=self.optim._max_grad_norm,
                                   log_tau=float(self.policy._log_tau), imitation_logits_penalty=float(self._weight_reg))
                eng = BQ.BCQEngine(c, h, w, n_act, BQ.flat_from_torch([p.detach() for p in params], *dims, dev), cfg)
                eng.iter = self._iter
                ms, vs, eng.adam_step = adam_state(self.optim._optim, params)
                eng.adam_m, eng.adam_v = BQ.flat_from_torch(ms, *dims, dev), BQ.flat_from_torch(vs, *dims, dev)
                eng.params_old = BQ.flat_from_torch([p.detach() for p in self._hip_old_params()], *dims, dev)
                self._hip_engine = eng
            return self._hip_engine

        def _hip_write_back(self) -> None:
            """Engine parameters, lagged parameters and Adam state -> the torch modules and torch.optim: fourteen tensors of the
            policy (the shared trunk is written once), the first ten of the lagged vector into `model_old`."""
            eng = self.__dict__.get("_hip_engine_obj")
            if eng is None:
                return
            dims = (eng.c, eng.h, eng.w, eng.n_act)
            params = params_by_keys(self.policy, BQ.TIANSHOU_KEYS)
            with torch.no_grad():
                for p, t in zip(params, BQ.flat_to_torch(eng.params, *dims)):
                    self._hip_put(p, t)
                for p, t in zip(self._hip_old_params(), BQ.flat_to_torch(eng.params_old, *dims)[:BQ.N_LAGGED]):
                    self._hip_put(p, t)
            store_adam_state(self.optim._optim, params, BQ.flat_to_torch(eng.adam_m, *dims), BQ.flat_to_torch(eng.adam_v, *dims),
                             eng.adam_step)

        def _preprocess_batch(self, batch, buffer, indices):
            c, h, w, self._hip_stack = self._layout(buffer, "HipDiscreteBCQ")
            _require_gpu(self._hip_device, "HipDiscreteBCQ")
            m = _mirror(self, buffer, self._hip_device)
            idx = self._hip_idx = torch.as_tensor(np.asarray(indices, np.int64), device=self._hip_device)
            eng = self._engine(c, h, w)
            self._hip_read_scalars(eng)
            batch.returns = eng.preprocess(m, m.obs, idx, self._hip_stack, obs_next_frames=m.obs_next)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            eng, m = self._hip_engine, self._hip_mirror
            obs = D.gather_obs_nhwc(m.obs, m, self._hip_idx, self._hip_stack, as_u8=True)
            act = torch.as_tensor(np.asarray(batch.act), device=self._hip_device)
            self._hip_read_scalars(eng)
            losses = eng.update_with_batch(obs, act, batch.returns)              # no batch.weight: BCQ reads and writes none
            self._iter = eng.iter
            self._hip_after_update()
            loss, q_loss, i_loss, reg_loss = losses.tolist()                      # one transfer for the four numbers
            return DiscreteBCQTrainingStats(loss=loss, q_loss=q_loss, i_loss=i_loss, reg_loss=reg_loss)   # discrete_bcq.py:256-261

        _layout = staticmethod(_q_layout)

    return HipDiscreteBCQ


def make_hip_discrete_crr(ref=None):
    """Returns HipDiscreteCRR(DiscreteCRR): `_update_with_batch` (imitation/discrete_crr.py:125-167) on the engine
    (tianshou_amd/crr.py).  Supported model: policy.actor = DiscreteActor(preprocess_net, hidden_sizes=[512],
    softmax_output=False) and critic = DiscreteCritic(preprocess_net, hidden_sizes=[512], last_size=n_act) on ONE shared
    DQNet(features_only=True), as examples/offline/atari_crr.py builds them, with one Adam over ModuleList([policy, critic]);
    buffer layouts as HipDQN -- a plain ReplayBuffer / VectorReplayBuffer; a prioritized one is accepted and its weights are
    ignored, as the reference ignores them.  `_preprocess_batch` is the base implementation unchanged (the discounted episodic
    returns nothing reads, and the return-standardization state) followed by the device mirror.  The mode, `_beta`,
    `_ratio_upper_bound`, `_min_q_weight` and gamma are read from the algorithm at every update; the statistics are
    DiscreteCRRTrainingStats(loss, actor_loss, critic_loss, cql_loss).  `actor_old` and `critic_old` each own a copy of the
    trunk; the reference syncs them together, so the engine keeps ONE lagged vector, refuses two lagged trunks that differ,
    and writes the lagged trunk back into both.  With target_update_freq == 0 there is no lagged state.  The collector's
    `policy.forward` stays on torch.  `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    from . import crr as CR
    from . import dqn as D

    Base = _ref(ref, "tianshou.algorithm.imitation.discrete_crr", "DiscreteCRR")
    DiscreteCRRTrainingStats = _ref(ref, "tianshou.algorithm.imitation.discrete_crr", "DiscreteCRRTrainingStats")
    supported = ("HipDiscreteCRR: policy.actor must be DiscreteActor(preprocess_net, hidden_sizes=[512], softmax_output=False) "
                 "and critic DiscreteCritic(preprocess_net, hidden_sizes=[512], last_size=n_act) on one shared "
                 "DQNet(features_only=True)")
    actor_keys = [k[len("0.actor."):] for k in CR.TIANSHOU_KEYS[:10]]                # actor_old: trunk + actor head
    critic_keys = actor_keys[:6] + [k[len("1."):] for k in CR.TIANSHOU_KEYS[10:]]     # critic_old: trunk + critic head

    class HipDiscreteCRR(_HipGlue, Base):
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            self._hip_check_model()
            _adam_of(self.optim)
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_live_params(self):
            named = dict(torch.nn.ModuleList([self.policy, self.critic]).named_parameters())
            if list(named.keys()) != CR.TIANSHOU_KEYS:
                raise NotImplementedError(f"{supported}; got parameters {list(named.keys())}")
            return [named[k] for k in CR.TIANSHOU_KEYS]

        def _hip_check_model(self) -> None:
            params = self._hip_live_params()
            actor = getattr(self.policy, "actor", None)
            if getattr(actor, "preprocess", None) is not getattr(self.critic, "preprocess", None):
                raise NotImplementedError(f"{supported}; the actor and the critic do not share one trunk object")
            shapes = [tuple(p.shape) for p in params]
            convs_ok = (len(shapes[0]) == 4 and shapes[0][0] == 32 and shapes[0][2:] == (8, 8) and shapes[2] == (64, 32, 4, 4)
                        and shapes[4] == (64, 64, 3, 3))
            if not convs_ok:
                raise NotImplementedError(f"{supported}; the preprocess_net is not the DQNet convolution trunk")
            for j in (6, 10):
                if shapes[j][0] != CR.HIDDEN or shapes[j + 2][1] != CR.HIDDEN:
                    raise NotImplementedError(f"{supported}; got hidden width {shapes[j][0]}")
            if shapes[8][0] != shapes[12][0] or not 1 <= shapes[8][0] <= 64:
                raise NotImplementedError("HipDiscreteCRR: both heads need the same number of actions, 1 <= n_act <= 64")
            if getattr(actor, "softmax_output", False):
                raise NotImplementedError(f"{supported}; got softmax_output=True")
            CR.mode_id(self._policy_improvement_mode)
            opt_params = [p for g in self.optim._optim.param_groups for p in g["params"]]
            if len(self.optim._optim.param_groups) != 1 or {id(p) for p in opt_params} != {id(p) for p in params}:
                raise NotImplementedError("HipDiscreteCRR: one optimizer group over the fourteen parameters of "
                                          "ModuleList([policy, critic])")

        def _hip_old_params(self):
            """The fourteen lagged parameters in TIANSHOU_KEYS order: the trunk and the actor head of `actor_old`, the critic
            head of `critic_old` (each the bare module or its EvalModeModuleWrapper), and `critic_old`'s own trunk, which must
            equal `actor_old`'s bit for bit -- the reference always syncs the two together."""
            a_old = params_by_keys(getattr(self.actor_old, "module", self.actor_old), actor_keys)
            c_old = params_by_keys(getattr(self.critic_old, "module", self.critic_old), critic_keys)
            if not all(torch.equal(x.detach(), y.detach()) for x, y in zip(a_old[:6], c_old[:6])):
                raise NotImplementedError("HipDiscreteCRR: the trunks of actor_old and critic_old differ; the engine keeps one "
                                          "lagged trunk (the reference syncs the two lagged networks together)")
            return a_old + c_old[6:]

        def _hip_read_scalars(self, eng) -> None:
            cfg = eng.cfg                                                         # read at every call, as the learning rate
            cfg.policy_improvement_mode = self._policy_improvement_mode
            cfg.beta, cfg.ratio_upper_bound = float(self._beta), float(self._ratio_upper_bound)
            cfg.min_q_weight, cfg.gamma = float(self._min_q_weight), float(self.discounted_return_computation.gamma)

        def _engine(self, c, h, w):
            if self._hip_engine is None:
                dev = self._hip_device
                params = self._hip_live_params()
                n_act = int(params[8].shape[0])
                dims = (c, h, w, n_act)
                _, g = _adam_of(self.optim)
                cfg = CR.CRRConfig(gamma=float(self.discounted_return_computation.gamma),
                                   policy_improvement_mode=self._policy_improvement_mode, beta=float(self._beta),
                                   ratio_upper_bound=float(self._ratio_upper_bound), min_q_weight=float(self._min_q_weight),
                                   target_update_freq=int(self._freq) if self._target else 0, lr=g["lr"],
                                   betas=tuple(g["betas"]), adam_eps=g["eps"], max_grad_norm=self.optim._max_grad_norm)
                eng = CR.CRREngine(c, h, w, n_act, CR.flat_from_torch([p.detach() for p in params], *dims, dev), cfg)
                eng.iter = self._iter
                ms, vs, eng.adam_step = adam_state(self.optim._optim, params)
                eng.adam_m, eng.adam_v = CR.flat_from_torch(ms, *dims, dev), CR.flat_from_torch(vs, *dims, dev)
                if self._target:
                    eng.params_old = CR.flat_from_torch([p.detach() for p in self._hip_old_params()], *dims, dev)
                self._hip_engine = eng
            return self._hip_engine

        def _hip_write_back(self) -> None:
            """Engine parameters, lagged parameters and Adam state -> the torch modules and torch.optim: fourteen live tensors
            (the shared trunk is written once); the lagged trunk into BOTH lagged modules, the lagged actor head into
            `actor_old`, the lagged critic head into `critic_old`.  Without lagged networks there is nothing more to write."""
            eng = self.__dict__.get("_hip_engine_obj")
            if eng is None:
                return
            dims = (eng.c, eng.h, eng.w, eng.n_act)
            params = self._hip_live_params()
            with torch.no_grad():
                for p, t in zip(params, CR.flat_to_torch(eng.params, *dims)):
                    self._hip_put(p, t)
                if self._target:
                    a_old = params_by_keys(getattr(self.actor_old, "module", self.actor_old), actor_keys)
                    c_old = params_by_keys(getattr(self.critic_old, "module", self.critic_old), critic_keys)
                    old = CR.flat_to_torch(eng.params_old, *dims)
                    for p, t in zip(a_old + c_old[6:] + c_old[:6], old + old[:6]):
                        self._hip_put(p, t)
            store_adam_state(self.optim._optim, params, CR.flat_to_torch(eng.adam_m, *dims), CR.flat_to_torch(eng.adam_v, *dims),
                             eng.adam_step)

        def _preprocess_batch(self, batch, buffer, indices):
            batch = super()._preprocess_batch(batch, buffer, indices)            # discrete_crr.py:113-123, on the host, unchanged
            c, h, w, self._hip_stack = self._layout(buffer, "HipDiscreteCRR")
            _require_gpu(self._hip_device, "HipDiscreteCRR")
            _mirror(self, buffer, self._hip_device)
            self._hip_idx = torch.as_tensor(np.asarray(indices, np.int64), device=self._hip_device)
            self._engine(c, h, w)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            eng, m, idx = self._hip_engine, self._hip_mirror, self._hip_idx
            obs = D.gather_obs_nhwc(m.obs, m, idx, self._hip_stack, as_u8=True)
            if m.obs_next is None:                                               # save_only_last_obs: the next slot's stack
                obs_next = D.gather_obs_nhwc(m.obs, m, m.next(idx), self._hip_stack, as_u8=True)
            else:
                obs_next = D.gather_obs_nhwc(m.obs_next, m, idx, self._hip_stack, as_u8=True)
            act = torch.as_tensor(np.asarray(batch.act), device=self._hip_device)
            self._hip_read_scalars(eng)
            losses = eng.update_with_batch(obs, obs_next, act, m.rew[idx].float(), m.done[idx])   # no batch.weight: CRR reads none
            self._iter = eng.iter
            self._hip_after_update()
            loss, actor_loss, critic_loss, cql_loss = losses.tolist()            # one transfer for the four numbers
            return DiscreteCRRTrainingStats(loss=loss, actor_loss=actor_loss, critic_loss=critic_loss,
                                            cql_loss=cql_loss)                   # discrete_crr.py:162-167

        _layout = staticmethod(_q_layout)

    return HipDiscreteCRR


def make_hip_rainbow(ref=None):
    """Returns HipRainbow(RainbowDQN): `_preprocess_batch` / `_update_with_batch` (dqn.py:257-275, rainbow.py:93-101 ->
    c51.py:120-160) on the engine.  Supported model: RainbowNet(is_dueling=True, is_noisy=True)
    (atari_network.py:154-208) with C51Policy's support, Adam; buffer layouts as HipDQN.  The NoisyLinear noise is drawn by
    the torch modules themselves (`RainbowDQN._sample_noise`, so torch's generator advances as in the reference) and
    handed to the engine.  `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    RainbowDQN = _ref(ref, "tianshou.algorithm.modelfree.rainbow", "RainbowDQN")
    LossSequenceTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "LossSequenceTrainingStats")

    from . import distq as Q
    from . import dqn as D
    from . import rainbow as RB

    class HipRainbow(_HipGlue, RainbowDQN):
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            keys = list(self.policy.model.state_dict().keys())
            if sorted(keys) != sorted(RB.TIANSHOU_KEYS + RB.NOISE_KEYS):
                raise NotImplementedError("HipRainbow: the model must be RainbowNet(is_dueling=True, is_noisy=True)")
            _adam_of(self.optim)
            self._hip_engine = None
            self._hip_glue_init()

        def _noise_of(self, model, dims):
            sd = model.state_dict()
            return RB.noise_from_torch([sd[k] for k in RB.NOISE_KEYS], *dims, self._hip_device)

        def _hip_qstate(self):
            return _QState(RB.TIANSHOU_KEYS, RB.flat_from_torch, RB.flat_to_torch,
                           lambda eng: (eng.c, eng.h, eng.w, eng.n_act, eng.cfg.n_atoms))

        def _engine(self, c, h, w):
            if self._hip_engine is None:
                model = self.policy.model
                n_atoms = int(self.policy.num_atoms)
                n_act = model.state_dict()["Q.2.mu_bias"].numel() // n_atoms
                dims = (c, h, w, n_act, n_atoms)
                cfg = Q.DistQConfig(kind=Q.C51, n_atoms=n_atoms, v_min=float(self.policy.v_min), v_max=float(self.policy.v_max),
                                    **_q_config_fields(self))
                eng = _q_load(self, RB.RainbowEngine(c, h, w, n_act, _q_flat(self, dims), self._noise_of(model, dims), cfg))
                if eng.params_old is not None:
                    eng.noise_old = self._noise_of(self.model_old, dims)
                self._hip_engine = eng
            return self._hip_engine

        def _preprocess_batch(self, batch, buffer, indices):
            c, h, w, self._hip_stack = self._layout(buffer, "HipRainbow")
            m, idx = _q_begin(self, "HipRainbow", batch, buffer, indices)
            batch.returns = self._engine(c, h, w).preprocess(m, idx)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            eng, m = self._hip_engine, self._hip_mirror
            idx, stack = self._hip_idx, self._hip_stack
            dims = (eng.c, eng.h, eng.w, eng.n_act, eng.cfg.n_atoms)
            self._sample_noise(self.policy.model)                                 # rainbow.py:97-100
            noise_old = None
            if self.use_target_network:
                self._sample_noise(self.model_old)
                noise_old = self._noise_of(self.model_old, dims)
            eng.set_noise(self._noise_of(self.policy.model, dims), noise_old)
            weight = batch.pop("weight", None)
            obs = D.gather_obs_nhwc(m.obs, m, idx, stack, as_u8=True)
            if m.obs_next is not None:                     # batch.obs_next = buffer[indices].obs_next (buffer_base.py:624-626)
                obs_next = D.gather_obs_nhwc(m.obs_next, m, idx, stack, as_u8=True)
            else:
                obs_next = D.gather_obs_nhwc(m.obs, m, m.next(idx), stack, as_u8=True)
            act = torch.as_tensor(np.asarray(batch.act), device=self._hip_device)
            loss, prio = eng.update_with_batch(obs, act, batch.returns, obs_next, weight)
            self._iter = eng.iter
            batch.weight = prio                                                   # prio-buffer, c51.py:157
            self._hip_after_update()
            return LossSequenceTrainingStats(loss=float(loss.item()))            # as c51.py:160

        _layout = staticmethod(_q_layout)

        def _hip_write_back(self) -> None:
            _q_write_back(self)
            eng = self.__dict__.get("_hip_engine_obj")
            if eng is not None and eng.params_old is not None and (eng.iter - 1) % eng.cfg.target_update_freq == 0:
                so, sn = self.model_old.state_dict(), self.policy.model.state_dict()      # the sync carried the noise along
                with torch.no_grad():
                    for k in RB.NOISE_KEYS:
                        so[k].copy_(sn[k])

    return HipRainbow



# ---------------------------------------------------------------------------------------------------
# SAC (sac.py:213-336) on the mujoco_sac.py networks
# ---------------------------------------------------------------------------------------------------
def _trunk_activation(mods, who: str) -> str:
    """The off-policy engines compute a `Net` trunk as Sequential(Linear, act, Linear, act, ...) with act = nn.ReLU -- `Net`'s
    default activation (utils/net/common.py:246-369) -- or nn.Tanh, the same for every network of the algorithm.  The state_dict
    keys only pin the Linear layers' positions; whatever sits between them (another activation, dropout, a norm layer without
    affine parameters) would be silently replaced, so the modules are checked here.  -> "relu" | "tanh"."""
    names = set()
    for mod in mods:
        seq = getattr(getattr(getattr(mod, "preprocess", None), "model", None), "model", None)
        ms = list(seq) if seq is not None else []
        ok = len(ms) >= 2 and len(ms) % 2 == 0 and all(
            type(ms[i]).__name__ in ("Linear", "EnsembleLinear") and type(ms[i + 1]) in (torch.nn.ReLU, torch.nn.Tanh) for i in range(0, len(ms), 2))
        if not ok:
            raise NotImplementedError(f"{who}: the trunk must be Net(hidden_sizes=[...]) with nn.ReLU or nn.Tanh after every Linear "
                                      f"layer (got {[type(m).__name__ for m in ms]})")
        names |= {"relu" if isinstance(ms[i], torch.nn.ReLU) else "tanh" for i in range(1, len(ms), 2)}
    if len(names) != 1:
        raise NotImplementedError(f"{who}: one activation class for all networks (got {sorted(names)})")
    return names.pop()


def _actor_bound(actor) -> float:
    """max_action of SAC's / REDQ's Gaussian actor for the engine: 0 for `unbounded=True` (examples/mujoco/mujoco_sac.py:88-94),
    `actor.max_action` for the class default `unbounded=False` (continuous.py:194, 230-231: mu = max_action * tanh(mu))."""
    return 0.0 if getattr(actor, "_unbounded", False) else float(getattr(actor, "max_action", 1.0))


def make_hip_sac(ref=None):
    """Returns HipSAC(SAC): `_preprocess_batch` / `_update_with_batch` (ddpg.py:287-301, sac.py:298-336) on the
    engine.  Supported nets: examples/mujoco/mujoco_sac.py:82-104 (Net[256, 256] ReLU, conditioned sigma,
    unbounded actor; concat critics);
    obs_next is the buffer's stored column or, with save_obs_next=False, obs[next(index)] (buffer_base.py:622-626).  rsample() noise: the engine's
    Philox stream by default, or (`update_noise="torch"`) torch's default generator on the host in the reference's order
    (target-policy call, then actor-loss call) -- the seed-exact mode the fixture replays use.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    SAC = _ref(ref, "tianshou.algorithm.modelfree.sac", "SAC")
    AutoAlpha = _ref(ref, "tianshou.algorithm.modelfree.sac", "AutoAlpha")
    SACTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.sac", "SACTrainingStats")
    Batch = _ref(ref, "tianshou.data", "Batch")

    from . import sac as S

    class HipSAC(_HipGlue, SAC):
        _HIP_LR = (("actor_lr", "policy_optim"), ("critic_lr", "critic_optim"), ("critic_lr", "critic2_optim"),
                   ("alpha_lr", "alpha"))
        def __init__(self, *args, device="cuda", data_parallel=False, group=None, allreduce=None, policy_forward="hip",
                     sampling="device", noise_seed=None, write_back="auto", update_noise="device", host_batch=False, **kwargs):
            """`data_parallel=True`: one process per GPU, every rank samples its own minibatch from its own buffer and
            `_update_with_batch` runs the four phases of `DataParallelSAC` around two all-reduces (critic gradients,
            actor gradient + mean log-probability); replicas stay identical, PER weights rank-local.
            `policy_forward="hip"`: `SACPolicy.forward` (sac.py:108-131) as the Collector calls it runs on
            `ts_sac_policy_forward_logits` with the engine's actor (`tianshou_amd.policy`; `sampling` / `noise_seed` as in
            HipPPO).
            Hook-level throughput (round 6; `bench.py --workload sac` `hook_level`): `write_back="auto"` keeps the updates in the
            engine until somebody reads the torch modules (lazy whenever the policy forward is the engine's; "eager" = after every
            update; `hip_sync()` forces it); `update_noise="device"` draws the two rsample() noises of an update from the
            engine's Philox stream instead of torch's host generator ("torch" = the reference's stream, seed-exact);
            `host_batch=False` lets `update()` sample indices only -- the hooks read the rows from the device mirror, the host
            copy `buffer.sample()` makes of them is never looked at (True: the reference's own `Algorithm._update`)."""
            super().__init__(*args, **kwargs)
            if update_noise not in ("device", "torch"):
                raise ValueError("update_noise must be 'device' or 'torch'")
            self._hip_update_noise, self._hip_host_batch, self._hip_noise_calls = update_noise, bool(host_batch), 0
            self._hip_noise_key = int(torch.initial_seed() % (2**31 - 1)) if noise_seed is None else int(noise_seed)
            self._hip_device = torch.device(device)
            keys = _ac_nets(self, "HipSAC", "networks must be those of examples/mujoco/mujoco_sac.py (Net trunks of one depth, "
                            "1 .. 6 hidden layers, single-Linear mu / sigma / Q heads)",
                            (("actor", self.policy.actor, S.actor_keys), ("critic1", self.critic, S.critic_keys),
                             ("critic2", self.critic2, S.critic_keys)), (self.policy_optim, self.critic_optim, self.critic2_optim))
            self._hip_akeys, self._hip_ckeys = keys["actor"], keys["critic1"]
            self._hip_bound = _actor_bound(self.policy.actor)
            self._hip_engine = None
            self._hip_glue_init()
            self._hip_dp_setup(data_parallel, group, allreduce, shard_buffer=False)
            if policy_forward not in ("hip", "torch"):
                raise ValueError("policy_forward must be 'hip' or 'torch'")
            if policy_forward == "hip":
                from . import policy as HP

                HP.attach(self.policy, "sac", self, device=str(self._hip_device), sampling=sampling, noise_seed=noise_seed,
                          obs_dim=self._hip_obs_dim, act_dim=self._hip_act_dim, hidden=self._hip_hidden, depth=self._hip_depth,
                          max_action=self._hip_bound, activation=self._hip_actfn)
            self._hip_set_write_back(write_back, attached=policy_forward == "hip")

        def update(self, buffer, sample_size):
            if self._hip_host_batch or buffer is None:
                return super().update(buffer, sample_size)
            return self._hip_offpolicy_update(buffer, sample_size, Batch)

        # The call counters of the two Philox streams (update noise, collector sampling noise) are run state outside the
        # reference's state_dict() format: saved / restored beside it, as HipPPO's shuffle key, so that a resumed run continues
        # both sequences instead of replaying them from call 1.
        def hip_extra_state(self) -> dict:
            return {"update_noise_calls": int(self._hip_noise_calls), **_policy_extra_state(self)}

        def load_hip_extra_state(self, state: dict) -> None:
            if "update_noise_calls" in state:
                self._hip_noise_calls = int(state["update_noise_calls"])
            _load_policy_extra_state(self, state)

        def _hip_rsample_noise(self, n, a):
            """eps of one Normal.rsample() call of the reference (sac.py:124-131): torch's host generator ("torch": the
            reference's own stream) or the engine's Philox stream keyed by (noise key, call number)."""
            if self._hip_update_noise == "torch":
                return torch.randn(n, a)
            from .buffer import normal_noise

            self._hip_noise_calls += 1
            return normal_noise((n, a), self._hip_noise_key ^ 0x5AC, self._hip_noise_calls, self._hip_device)

        def _engine(self):
            if self._hip_engine is None:
                flats = {p.name: p.flat() for p in self._hip_parts()}
                eng = S.SACEngine(self._hip_obs_dim, self._hip_act_dim, flats["actor"], flats["critic1"], flats["critic2"],
                                  S.SACConfig(**_ac_config_fields(self), **_ac_entropy_fields(self, AutoAlpha)),
                                  hidden=self._hip_hidden, depth=self._hip_depth, max_action=self._hip_bound, activation=self._hip_actfn)
                self._hip_engine = _ac_load(self, eng)     # resume: lagged critics, Adam moments / steps of a loaded checkpoint
            return self._hip_engine

        def _hip_parts(self):
            o, a, h, dev, sz = self._hip_obs_dim, self._hip_act_dim, self._hip_hidden, self._hip_device, self._hip_sizes

            def part(name, mod, old, optim, keys, fwd, back):
                return _ACPart(name, mod, old, optim, keys, lambda t: fwd(t, o, a, dev, hidden=h),
                               lambda f: back(f, o, a, h, sizes=sz[name]), "adam_step", True)

            return (part("actor", self.policy.actor, None, self.policy_optim, self._hip_akeys, S.actor_flat_from_torch, S.actor_flat_to_torch),
                    part("critic1", self.critic, self.critic_old.module, self.critic_optim, self._hip_ckeys,
                         S.critic_flat_from_torch, S.critic_flat_to_torch),
                    part("critic2", self.critic2, self.critic2_old.module, self.critic2_optim, self._hip_ckeys,
                         S.critic_flat_from_torch, S.critic_flat_to_torch))

        def _preprocess_batch(self, batch, buffer, indices):
            eng, m, idx = _ac_begin(self, "HipSAC", buffer, indices)
            # Inside HipSAC.update()'s own sequence (`_hip_offpolicy_update`: nobody reads the batch between the two hooks) an
            # n_step = 1 update with the engine's noise is ONE library call, made by `_update_with_batch` (ts_sac_learn_rows: the
            # target pass in front of the update, 16 launches instead of 22); `batch.returns` is attached there.  Called on its own
            # (the reference's `_update`, `host_batch=True`, "torch" noise, data parallel) the hook computes the returns here.
            self.__dict__["_hip_deferred"] = (self.__dict__.get("_hip_own_sequence", False) and self._hip_update_noise == "device"
                                              and not self._hip_dp_on and eng.cfg.n_step == 1 and eng._rows_ok(m)
                                              and not os.environ.get("TS_SAC_TWO_CALLS"))
            if self.__dict__["_hip_deferred"]:
                return batch
            noise = self._hip_rsample_noise(len(indices), eng.act_dim)      # Normal.rsample of the target policy call
            batch.returns = eng.preprocess(m, idx, noise).reshape(-1, 1)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            from .buffer import gather_rows_multi

            eng, m = self._hip_engine, self._hip_mirror
            weight = getattr(batch, "weight", None)
            if self.__dict__.pop("_hip_deferred", False):
                # target pass + update as one call; the two rsample() draws keep their call numbers (target: c + 1, update: c + 2)
                key, c = self._hip_noise_key ^ 0x5AC, self._hip_noise_calls
                self._hip_noise_calls += 2
                stats, w, ret, _ = eng.learn_rows(m, self._hip_idx, noise_key=(key, c + 1), weight=weight, noise_streams=2)
                batch.returns = ret.reshape(-1, 1)
            else:
                noise = self._hip_rsample_noise(int(self._hip_idx.numel()), eng.act_dim)
                runner = eng
                if self._hip_dp_on:
                    from .distributed import DataParallelSAC

                    runner = self._hip_dp(DataParallelSAC, eng)
                if runner is eng and hasattr(eng, "update_with_rows"):           # the input packing reads the mirror's rows
                    stats, w = eng.update_with_rows(m, self._hip_idx, batch.returns.reshape(-1), noise, weight)
                else:
                    stats, w = runner.update_with_batch(*gather_rows_multi([m.obs, m.act], self._hip_idx),
                                                        batch.returns.reshape(-1), noise, weight)
            batch.weight = w                                                      # prio-buffer, sac.py:306
            s = stats.cpu().numpy()                                               # one D2H per update()
            self._hip_after_update()                                              # write-back now ("eager") or when read ("lazy")
            auto = eng.cfg.auto_alpha
            return SACTrainingStats(actor_loss=float(s[0]), critic1_loss=float(s[1]), critic2_loss=float(s[2]),
                                    alpha=float(s[3]), alpha_loss=float(s[4]) if auto else None)

        _hip_write_back = _ac_write_back

    return HipSAC


# ---------------------------------------------------------------------------------------------------
# REDQ (redq.py) on the nets of test/continuous/test_redq.py
# ---------------------------------------------------------------------------------------------------
def make_hip_redq(ref=None):
    """Returns HipREDQ(REDQ): `_preprocess_batch` / `_update_with_batch` (ddpg.py:287-301, redq.py:248-304) on the engine.
    Supported nets: SAC's actor (Net[256, 256] ReLU, conditioned sigma, unbounded) and one critic module made of
    EnsembleLinear layers with hidden [256, 256] (test/continuous/test_redq.py:86-107);
    obs_next is the buffer's stored column or, with save_obs_next=False, obs[next(index)] (buffer_base.py:622-626).
    The rsample() noise comes from torch's default generator and the critic subset from NumPy's global generator, in
    the reference's order (target call: noise, then np.random.choice; actor step: noise).
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    REDQ = _ref(ref, "tianshou.algorithm.modelfree.redq", "REDQ")
    REDQTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.redq", "REDQTrainingStats")
    AutoAlpha = _ref(ref, "tianshou.algorithm.modelfree.sac", "AutoAlpha")

    from . import redq as RQ
    from . import sac as S

    class HipREDQ(_HipGlue, REDQ):
        _HIP_LR = (("actor_lr", "policy_optim"), ("critic_lr", "critic_optim"), ("alpha_lr", "alpha"))
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)

            def ensemble_widths(t):                                   # EnsembleLinear weights [E, in, out]
                cw = t[:-2:2]
                if any(w.dim() != 3 or w.shape[0] != self.ensemble_size or (i > 0 and w.shape[1] != cw[i - 1].shape[2]) for i, w in enumerate(cw)):
                    raise NotImplementedError("EnsembleLinear weights [ensemble_size, in, out] are required")
                return tuple(int(w.shape[2]) for w in cw)

            keys = _ac_nets(self, "HipREDQ", "networks must be those of test/continuous/test_redq.py (SAC's actor; a critic of "
                            "EnsembleLinear layers; trunks of one depth, 1 .. 6 hidden layers)",
                            (("actor", self.policy.actor, S.actor_keys), ("critic", self.critic, RQ.critic_keys)),
                            (self.policy_optim, self.critic_optim), widths={"critic": ensemble_widths})
            self._hip_akeys, self._hip_ckeys = keys["actor"], keys["critic"]
            self._hip_bound = _actor_bound(self.policy.actor)
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_parts(self):
            o, a, h, dev, sz = self._hip_obs_dim, self._hip_act_dim, self._hip_hidden, self._hip_device, self._hip_sizes
            E = self.ensemble_size
            return (_ACPart("actor", self.policy.actor, None, self.policy_optim, self._hip_akeys,
                            lambda t: S.actor_flat_from_torch(t, o, a, dev, hidden=h),
                            lambda f: S.actor_flat_to_torch(f, o, a, h, sizes=sz["actor"]), "actor_steps", True),
                    _ACPart("critics", self.critic, self.critic_old.module, self.critic_optim, self._hip_ckeys,
                            lambda t: RQ.ensemble_flat_from_torch(t, o, a, dev, hidden=h),
                            lambda f: RQ.ensemble_flat_to_torch(f, E, o, a, h, sizes=sz["critic"]), "critic_gradient_step", False))

        def _engine(self):
            if self._hip_engine is None:
                cfg = RQ.REDQConfig(**_ac_config_fields(self), **_ac_entropy_fields(self, AutoAlpha), ensemble_size=self.ensemble_size,
                                    subset_size=self.subset_size, actor_delay=self.actor_delay, target_mode=self.target_mode)
                flats = {p.name: p.flat() for p in self._hip_parts()}
                eng = RQ.REDQEngine(self._hip_obs_dim, self._hip_act_dim, flats["actor"], flats["critics"], cfg, hidden=self._hip_hidden,
                                    depth=self._hip_depth, max_action=self._hip_bound, activation=self._hip_actfn)
                # resume: the counters the reference keeps on the algorithm, then lagged ensemble, Adam moments / actor steps
                eng.critic_gradient_step = int(self.critic_gradient_step)
                eng._stats[0] = float(self._last_actor_loss)
                self._hip_engine = _ac_load(self, eng)
            return self._hip_engine

        def _preprocess_batch(self, batch, buffer, indices):
            eng, m, idx = _ac_begin(self, "HipREDQ", buffer, indices)
            noise = torch.randn(len(indices), eng.act_dim)                  # Normal.rsample of the target policy call
            subset = np.random.choice(self.ensemble_size, self.subset_size, replace=False)     # redq.py:252
            batch.returns = eng.preprocess(m, idx, noise, subset).reshape(-1, 1)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            from .buffer import gather_rows_multi

            eng, m = self._hip_engine, self._hip_mirror
            weight = getattr(batch, "weight", None)
            did_actor = eng.will_update_actor()
            noise = torch.randn(len(batch), eng.act_dim) if did_actor else None
            stats, w = eng.update_with_batch(*gather_rows_multi([m.obs, m.act], self._hip_idx),
                                             batch.returns.reshape(-1), noise, weight)
            batch.weight = w                                                      # prio-buffer, redq.py:272
            s = stats.cpu().numpy()                                               # one D2H per update()
            self.critic_gradient_step = eng.critic_gradient_step
            self._last_actor_loss = float(s[0])
            self._hip_after_update()
            return REDQTrainingStats(actor_loss=float(s[0]), critic_loss=float(s[1]), alpha=float(s[2]),
                                     alpha_loss=None if np.isnan(s[3]) else float(s[3]))

        _hip_write_back = _ac_write_back

    return HipREDQ


# ---------------------------------------------------------------------------------------------------
# DiscreteSAC (discrete_sac.py) on the MLP nets of test/discrete/test_discrete_sac.py
# ---------------------------------------------------------------------------------------------------
def make_hip_discrete_sac(ref=None):
    """Returns HipDiscreteSAC(DiscreteSAC): `_preprocess_batch` / `_update_with_batch` (ddpg.py:287-301,
    discrete_sac.py:147-196) on the engine.  Supported nets: Net(obs, [h, h]) ReLU under DiscreteActor(softmax_output=
    False) and DiscreteCritic(last_size=n_act) (test/discrete/test_discrete_sac.py:88-97), h a multiple of 32; the
    obs_next is the buffer's stored column or obs[next(index)] (buffer_base.py:622-626).  `match_rng_stream`: the reference's two policy calls per update draw
    `Categorical.sample()` values that are never used; with the flag set (default) the same draws are made from the
    engine's logits so that torch's global generator advances exactly as in the reference.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    from torch.distributions import Categorical

    DiscreteSAC = _ref(ref, "tianshou.algorithm.modelfree.discrete_sac", "DiscreteSAC")
    DiscreteSACTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.discrete_sac", "DiscreteSACTrainingStats")
    AutoAlpha = _ref(ref, "tianshou.algorithm.modelfree.sac", "AutoAlpha")

    from . import dsac as DS
    from .sac import SACConfig

    class HipDiscreteSAC(_HipGlue, DiscreteSAC):
        _HIP_LR = (("actor_lr", "policy_optim"), ("critic_lr", "critic_optim"), ("critic_lr", "critic2_optim"),
                   ("alpha_lr", "alpha"))
        def __init__(self, *args, device="cuda", match_rng_stream: bool = True, **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            self._hip_match_rng = match_rng_stream
            keys = _ac_nets(self, "HipDiscreteSAC", "networks must be Net(obs, [h, ...]) of one depth (1 .. 6 hidden layers) + a "
                            "single Linear head",
                            (("actor", self.policy.actor, DS.net_keys), ("critic1", self.critic, DS.net_keys),
                             ("critic2", self.critic2, DS.net_keys)), (self.policy_optim, self.critic_optim, self.critic2_optim))
            self._hip_keys = keys["actor"]
            if not 2 <= self._hip_act_dim <= 64:
                raise NotImplementedError("HipDiscreteSAC: 2..64 actions")
            if getattr(self.policy.actor, "softmax_output", False):
                raise NotImplementedError("HipDiscreteSAC: the actor must output logits (softmax_output=False)")
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_parts(self):
            o, n, h, dev, sz = self._hip_obs_dim, self._hip_act_dim, self._hip_hidden, self._hip_device, self._hip_sizes

            def part(name, mod, old, optim):
                return _ACPart(name, mod, old, optim, self._hip_keys, lambda t: DS.net_flat_from_torch(t, o, n, h, dev),
                               lambda f: DS.net_flat_to_torch(f, o, n, h, sizes=sz[name]), "adam_step", True)

            return (part("actor", self.policy.actor, None, self.policy_optim),
                    part("critic1", self.critic, self.critic_old.module, self.critic_optim),
                    part("critic2", self.critic2, self.critic2_old.module, self.critic2_optim))

        def _engine(self):
            if self._hip_engine is None:
                flats = {p.name: p.flat() for p in self._hip_parts()}
                eng = DS.DiscreteSACEngine(self._hip_obs_dim, self._hip_act_dim, self._hip_hidden, flats["actor"], flats["critic1"],
                                           flats["critic2"], SACConfig(**_ac_config_fields(self), **_ac_entropy_fields(self, AutoAlpha)),
                                           depth=self._hip_depth, activation=self._hip_actfn)
                self._hip_engine = _ac_load(self, eng)                 # resume from a loaded checkpoint
            return self._hip_engine

        def _hip_draw(self, obs):
            if self._hip_match_rng:                  # discrete_sac.py:60-66: dist.sample() inside the training step
                Categorical(logits=self._hip_engine.policy_forward(obs).cpu()).sample()

        def _preprocess_batch(self, batch, buffer, indices):
            from .buffer import gather_rows

            eng, m, idx = _ac_begin(self, "HipDiscreteSAC", buffer, indices)
            if self._hip_match_rng:
                from .returns import nstep_indices

                self._hip_draw(gather_rows(m.obs_next, nstep_indices(m, idx, eng.cfg.n_step)))
            batch.returns = eng.preprocess(m, idx).reshape(-1, 1)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            from .buffer import gather_rows

            eng, m = self._hip_engine, self._hip_mirror
            weight = getattr(batch, "weight", None)
            obs = gather_rows(m.obs, self._hip_idx)
            self._hip_draw(obs)
            stats, w = eng.update_with_batch(obs, gather_rows(m.act, self._hip_idx), batch.returns.reshape(-1), weight)
            batch.weight = w                                                      # prio-buffer, discrete_sac.py:174
            s = stats.cpu().numpy()                                               # one D2H per update()
            self._hip_after_update()
            auto = eng.cfg.auto_alpha
            return DiscreteSACTrainingStats(actor_loss=float(s[0]), critic1_loss=float(s[1]), critic2_loss=float(s[2]),
                                            alpha=float(s[3]), alpha_loss=float(s[4]) if auto else None)

        _hip_write_back = _ac_write_back

    return HipDiscreteSAC


def make_hip_discrete_sac_cnn(ref=None):
    """Returns HipDiscreteSACCnn(DiscreteSAC): `_preprocess_batch` / `_update_with_batch` (ddpg.py:287-301,
    discrete_sac.py:147-196) on the engine (tianshou_amd/dsac_cnn.py) for the networks of examples/atari/atari_sac.py:
    DiscreteActor(softmax_output=False), DiscreteCritic(last_size=n_act) and a second, explicitly given DiscreteCritic, single
    Linear heads on ONE shared DQNet(features_only=True, output_dim_added_layer=H), H a multiple of 32 in [32, 1024]; Adam on
    all three optimizers (each over the shared trunk and its own head, no gradient clipping) and on AutoAlpha; anything else
    raises NotImplementedError naming what is unsupported.  The trunk is stepped three times per update with three moment sets,
    as the reference's three optimizers step it.  `critic_old` and `critic2_old` each own a trunk copy that the reference keeps
    bit-equal; the engine keeps ONE lagged trunk, refuses two lagged trunks that differ and writes the lagged trunk back into
    both.  Buffer layouts as HipDQN / HipIQN (whole [c, h, w] observations, or single frames with `stack_num`); a prioritized
    buffer's weights go in and `batch.weight` = (td1 + td2) / 2 comes out.  `match_rng_stream` as in HipDiscreteSAC.  The
    collector's `policy.forward` stays on torch.  `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    from torch.distributions import Categorical

    DiscreteSAC = _ref(ref, "tianshou.algorithm.modelfree.discrete_sac", "DiscreteSAC")
    DiscreteSACTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.discrete_sac", "DiscreteSACTrainingStats")
    AutoAlpha = _ref(ref, "tianshou.algorithm.modelfree.sac", "AutoAlpha")

    from . import dqn as D
    from . import dsac_cnn as DC
    from .sac import SACConfig

    who = "HipDiscreteSACCnn"
    supported = (f"{who}: policy.actor must be DiscreteActor(preprocess_net, softmax_output=False), critic and critic2 "
                 "DiscreteCritic(preprocess_net, last_size=n_act), single Linear heads on one shared "
                 "DQNet(features_only=True, output_dim_added_layer=H)")
    set_keys = DC.TRUNK_KEYS + DC.HEAD_KEYS                                   # one module's ten tensors: trunk + own head

    class HipDiscreteSACCnn(_HipGlue, DiscreteSAC):
        _HIP_LR = (("actor_lr", "policy_optim"), ("critic_lr", "critic_optim"), ("critic_lr", "critic2_optim"),
                   ("alpha_lr", "alpha"))

        def __init__(self, *args, device="cuda", match_rng_stream: bool = True, **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            self._hip_match_rng = match_rng_stream
            self._hip_check_model()
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_live_params(self):
            named = dict(torch.nn.ModuleList([self.policy, self.critic, self.critic2]).named_parameters())
            if list(named.keys()) != DC.TIANSHOU_KEYS:
                raise NotImplementedError(f"{supported}; got parameters {list(named.keys())}")
            return [named[k] for k in DC.TIANSHOU_KEYS]

        def _hip_sets(self):
            """(optimizer wrapper, its ten parameters: the shared trunk and the own head) in the engine's SETS order."""
            p = self._hip_live_params()
            return ((self.critic_optim, p[:8] + p[10:12]), (self.critic2_optim, p[:8] + p[12:14]), (self.policy_optim, p[:10]))

        def _hip_check_model(self) -> None:
            actor = getattr(self.policy, "actor", None)
            trunks = [getattr(m, "preprocess", None) for m in (actor, self.critic, self.critic2)]
            if trunks[0] is None or trunks[1] is not trunks[0]:
                raise NotImplementedError(f"{supported}; the actor and the critic do not share one feature-net object")
            if trunks[2] is not trunks[0]:
                raise NotImplementedError(f"{supported}; critic2 does not share the feature-net object (critic2=None deep-copies "
                                          "the first critic and its trunk, which is a different network: pass critic2 explicitly)")
            params = self._hip_live_params()
            shapes = [tuple(p.shape) for p in params]
            convs_ok = (len(shapes[0]) == 4 and shapes[0][0] == 32 and shapes[0][2:] == (8, 8) and shapes[2] == (64, 32, 4, 4)
                        and shapes[4] == (64, 64, 3, 3))
            if not convs_ok or len(shapes[6]) != 2:
                raise NotImplementedError(f"{supported}; the preprocess_net is not the DQNet convolution trunk with an added layer")
            # the kernel shapes do not tell the strides: the engine computes stride 4 / 2 / 1 without padding, and nothing else
            convs = [m for m in trunks[0].modules() if isinstance(m, torch.nn.Conv2d)]
            got = [(m.kernel_size, m.stride, m.padding, m.dilation, m.groups) for m in convs]
            if got != [((k, k), (st, st), (0, 0), (1, 1), 1) for k, st in ((8, 4), (4, 2), (3, 1))]:
                raise NotImplementedError(f"{supported}; the convolutions must be DQNet's (kernel 8 / 4 / 3, stride 4 / 2 / 1, no "
                                          f"padding, dilation or groups), got (kernel, stride, padding, dilation, groups) {got}")
            mods = [m for m in trunks[0].modules() if not list(m.children())]
            kinds = [type(m).__name__ for m in mods]
            if kinds != ["Conv2d", "ReLU", "Conv2d", "ReLU", "Conv2d", "ReLU", "Flatten", "Linear", "ReLU"]:
                raise NotImplementedError(f"{supported}; the preprocess_net must be DQNet's chain conv, ReLU, conv, ReLU, conv, "
                                          f"ReLU, Flatten, Linear, ReLU on the raw pixel values, got {kinds}")
            hidden = shapes[6][0]
            if hidden % 32 or not 32 <= hidden <= 1024:
                raise NotImplementedError(f"{who}: output_dim_added_layer must be a multiple of 32 in [32, 1024], got {hidden}")
            n_act = shapes[8][0]
            if any(shapes[j] != (n_act, hidden) for j in (8, 10, 12)) or not 1 <= n_act <= 64:
                raise NotImplementedError(f"{who}: the three heads must be Linear({hidden}, n_act) with the same 1 <= n_act <= 64")
            if getattr(actor, "softmax_output", False):
                raise NotImplementedError(f"{supported}; got softmax_output=True")
            for name, (opt, own) in zip(("critic_optim", "critic2_optim", "policy_optim"), self._hip_sets()):
                o, _ = _adam_of(opt)
                if opt._max_grad_norm:
                    raise NotImplementedError(f"{who}: {name} clips the gradient norm; the engine steps without clipping")
                if {id(p) for g in o.param_groups for p in g["params"]} != {id(p) for p in own}:
                    raise NotImplementedError(f"{who}: {name} must hold the shared trunk and its own head, ten tensors")
            if isinstance(self.alpha, AutoAlpha):
                o = self.alpha._optim
                g = o.param_groups[0]
                if type(o).__name__ != "Adam" or g.get("weight_decay", 0) != 0 or g.get("amsgrad", False):
                    raise NotImplementedError(f"{who}: AutoAlpha must use torch.optim.Adam without weight decay / amsgrad")
            self._hip_hidden, self._hip_n_act = int(hidden), int(n_act)

        def _hip_old_modules(self):
            return [getattr(m, "module", m) for m in (self.critic_old, self.critic2_old)]

        def _hip_old_params(self):
            """The lagged vector's twelve tensors: the trunk and the head of `critic_old`, the head of `critic2_old`, whose own
            trunk must equal `critic_old`'s bit for bit -- the reference moves both with the same tau from the same live trunk."""
            o1, o2 = (params_by_keys(m, set_keys) for m in self._hip_old_modules())
            if not all(torch.equal(x.detach(), y.detach()) for x, y in zip(o1[:8], o2[:8])):
                raise NotImplementedError(f"{who}: the trunks of critic_old and critic2_old differ; the engine keeps one lagged "
                                          "trunk (the reference averages both from the same live trunk with the same tau)")
            return o1 + o2[8:]

        def _engine(self, c, h, w):
            if self._hip_engine is None:
                dev, hid, n_act = self._hip_device, self._hip_hidden, self._hip_n_act
                dims = (c, h, w, n_act, hid)
                cfg = SACConfig(**_ac_config_fields(self), **_ac_entropy_fields(self, AutoAlpha))
                eng = DC.DiscreteSACCnnEngine(c, h, w, n_act, hid,
                                              DC.flat_from_torch([p.detach() for p in self._hip_live_params()], *dims, dev), cfg)
                eng.params_old = DC.flat_from_torch([p.detach() for p in self._hip_old_params()], *dims, dev)
                for k, (opt, own) in enumerate(self._hip_sets()):          # resume from a loaded checkpoint
                    ms, vs, step = adam_state(opt._optim, own)
                    eng.adam_m[k], eng.adam_v[k] = DC.flat_from_torch(ms, *dims, dev), DC.flat_from_torch(vs, *dims, dev)
                    eng.adam_step = max(eng.adam_step, step)
                if cfg.auto_alpha:
                    st = self.alpha._optim.state.get(self.alpha._log_alpha, {})
                    if "exp_avg" in st:
                        eng.log_alpha_m[0], eng.log_alpha_v[0] = float(st["exp_avg"]), float(st["exp_avg_sq"])
                self._hip_engine = eng
            return self._hip_engine

        def _hip_write_back(self) -> None:
            """Engine state -> the torch modules and torch.optim: fourteen live tensors (the shared trunk once); the ONE lagged
            trunk into both lagged modules, each lagged head into its own; the three optimizers' moments over trunk + own head
            and the shared step count; log alpha and its optimizer."""
            eng = self.__dict__.get("_hip_engine_obj")
            if eng is None:
                return
            dims = (eng.c, eng.h, eng.w, eng.n_act, eng.hidden)
            with torch.no_grad():
                for p, t in zip(self._hip_live_params(), DC.flat_to_torch(eng.params, *dims)):
                    self._hip_put(p, t)
                old = DC.flat_to_torch(eng.params_old, *dims)
                o1, o2 = (params_by_keys(m, set_keys) for m in self._hip_old_modules())
                for p, t in zip(o1 + o2, old[:10] + old[:8] + old[10:12]):
                    self._hip_put(p, t)
                if eng.adam_step:
                    for k, (opt, own) in enumerate(self._hip_sets()):
                        store_adam_state(opt._optim, own, DC.flat_to_torch(eng.adam_m[k], *dims),
                                         DC.flat_to_torch(eng.adam_v[k], *dims), eng.adam_step)
                if eng.cfg.auto_alpha:
                    self._hip_put(self.alpha._log_alpha, eng.log_alpha[0])
                    if eng.adam_step:
                        store_adam_state(self.alpha._optim, [self.alpha._log_alpha], [eng.log_alpha_m[0]], [eng.log_alpha_v[0]],
                                         eng.adam_step)

        def _hip_draw(self, obs):
            if self._hip_match_rng:                  # discrete_sac.py:74-78: dist.sample() inside the training step
                Categorical(logits=self._hip_engine.policy_forward(obs).cpu()).sample()

        def _preprocess_batch(self, batch, buffer, indices):
            c, h, w, self._hip_stack = self._layout(buffer, who)
            m, idx = _q_begin(self, who, batch, buffer, indices)
            eng = self._engine(c, h, w)
            if self._hip_match_rng:
                from .returns import nstep_indices

                after = nstep_indices(m, idx, eng.cfg.n_step)
                if m.obs_next is None:
                    self._hip_draw(D.gather_obs_nhwc(m.obs, m, m.next(after), self._hip_stack, as_u8=True))
                else:
                    self._hip_draw(D.gather_obs_nhwc(m.obs_next, m, after, self._hip_stack, as_u8=True))
            batch.returns = eng.preprocess(m, m.obs, idx, self._hip_stack, obs_next_frames=m.obs_next).reshape(-1, 1)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            eng, m = self._hip_engine, self._hip_mirror
            weight = getattr(batch, "weight", None)
            obs = D.gather_obs_nhwc(m.obs, m, self._hip_idx, self._hip_stack, as_u8=True)
            self._hip_draw(obs)
            act = torch.as_tensor(np.asarray(batch.act), device=self._hip_device)
            stats, w = eng.update_with_batch(obs, act, batch.returns.reshape(-1), weight)
            batch.weight = w                                                      # prio-buffer, discrete_sac.py:174
            s = stats.cpu().numpy()                                               # one D2H per update()
            self._hip_after_update()
            auto = eng.cfg.auto_alpha
            return DiscreteSACTrainingStats(actor_loss=float(s[0]), critic1_loss=float(s[1]), critic2_loss=float(s[2]),
                                            alpha=float(s[3]), alpha_loss=float(s[4]) if auto else None)

        _layout = staticmethod(_q_layout)

    return HipDiscreteSACCnn


# ---------------------------------------------------------------------------------------------------
# PPO on the Atari actor-critic (examples/atari/atari_ppo.py:106-135)
# ---------------------------------------------------------------------------------------------------
def make_hip_ppo_cnn(algo: str = "ppo", ref=None):
    """Returns HipPPOCnn(PPO) for DQNet(features_only=True, output_dim_added_layer=512) shared by
    DiscreteActor(softmax_output=False) and DiscreteCritic; Categorical policy; Adam.  algo="a2c": HipA2CCnn(A2C).
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    A2CTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.a2c", "A2CTrainingStats")
    SequenceSummaryStats = _ref(ref, "tianshou.data", "SequenceSummaryStats")
    PPO = _on_policy_base(algo, ref)

    from . import ppo_cnn as PC

    class HipPPOCnn(_HipGlue, PPO):
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            actor, critic = self.policy.actor, self.critic
            sa, sc = actor.state_dict(), critic.state_dict()
            if list(sa.keys()) != PC.TRUNK_KEYS + PC.HEAD_KEYS or list(sc.keys()) != PC.TRUNK_KEYS + PC.HEAD_KEYS \
                    or actor.preprocess is not critic.preprocess or getattr(actor, "softmax_output", True):
                raise NotImplementedError("HipPPOCnn: actor / critic must share one DQNet(features_only=True, "
                                          "output_dim_added_layer=512) trunk with single-Linear heads (logits)")
            optimizer_fields(self.optim._optim)                # Adam / RMSprop incl. weight decay (ts::optim_step)
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_params(self):
            return params_by_keys(self.policy.actor, PC.TRUNK_KEYS + PC.HEAD_KEYS) + params_by_keys(self.critic, PC.HEAD_KEYS)

        def _layout(self, buffer):
            obs = np.asarray(buffer.obs)
            stack = int(getattr(buffer, "stack_num", 1))
            if stack > 1:
                return stack, obs.shape[1], obs.shape[2], stack
            if obs.ndim != 4:
                raise NotImplementedError("HipPPOCnn: observations must be [c, h, w]")
            return obs.shape[1], obs.shape[2], obs.shape[3], 1

        def _hip_parts(self, eng=None, frame=None):
            """`frame`: (c, h, w) of the buffer's observations, before the engine exists."""
            params, dev = self._hip_params(), self._hip_device
            dims = (*(frame or (eng.c, eng.h, eng.w)), params[8].shape[0])
            return [_OnPart("params", ("adam_m", "adam_v"), self.optim, params,
                            lambda t: PC.flat_from_torch(t, *dims, dev), lambda f: PC.flat_to_torch(f, *dims))]

        def _engine(self, c, h, w):
            if self._hip_engine is None:
                part, = self._hip_parts(frame=(c, h, w))
                eng = PC.CnnPPOEngine(c, h, w, part.params[8].shape[0], part.flat(), ppo_config_from(self))
                self._hip_engine = _on_load(self, eng)
            return self._hip_engine

        _hip_write_back = _on_write_back

        def _hip_rewards(self, eng, m):
            """The rewards the returns are computed from, in sample_indices(0) order: None = the mirror's column, read in place
            (a reward-supplying wrapper -- HipICMCnn -- leaves its float64 device tensor in `_hip_rew_source` for one call)."""
            return self.__dict__.get("_hip_rew_source")

        def _preprocess_batch(self, batch, buffer, indices):
            _require_gpu(self._hip_device, "HipPPOCnn")
            c, h, w, stack = self._layout(buffer)
            eng = self._engine(c, h, w)
            m = _mirror(self, buffer, self._hip_device)
            rew = self._hip_rewards(eng, m)
            kw = {} if rew is None else {"rew": rew}
            pre = eng.preprocess(m, m.obs, m.act, stack, obs_next_frames=m.obs_next, **kw)
            self._hip_pre, self._hip_stack = pre, stack
            batch.v_s, batch.returns, batch.adv, batch.logp_old = pre["v_s"], pre["returns"], pre["adv"], pre["logp_old"]
            return batch

        def _update_with_batch(self, batch, batch_size, repeat):
            self._hip_refresh_lr()
            eng, m = self._hip_engine, self._hip_mirror
            perms = [np.random.permutation(len(batch)) for _ in range(repeat)]     # Batch.split, batch.py:1209
            losses, steps = eng.update(m, m.obs, self._hip_pre, self._hip_stack, batch_size, repeat, perms)
            self._hip_write_back()
            return _a2c_stats(A2CTrainingStats, SequenceSummaryStats.from_sequence, losses, steps)

    if algo == "a2c":
        HipPPOCnn.__name__ = HipPPOCnn.__qualname__ = "HipA2CCnn"
    return HipPPOCnn


# ---------------------------------------------------------------------------------------------------
# PPO on the CartPole-shape networks (BASELINE.json configs[0], test/discrete/test_ppo_discrete.py:88-127)
# ---------------------------------------------------------------------------------------------------
def make_hip_ppo_discrete(algo: str = "ppo", ref=None):
    """Returns HipPPODiscrete(PPO) for Net(obs, [h, h]) shared by DiscreteActor and DiscreteCritic, Categorical policy
    (`softmax_output=True` with `dist_fn=torch.distributions.Categorical`, or `softmax_output=False` with the default
    logits dist_fn), Adam; h a multiple of 32, at most 31 actions;
    obs_next is the buffer's stored column or, with save_obs_next=False, obs[next(index)] (buffer_base.py:622-626).
    algo="a2c": HipA2CDiscrete(A2C).  `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    from torch.distributions import Categorical

    A2CTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.a2c", "A2CTrainingStats")
    dist_fn_categorical_from_logits = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "dist_fn_categorical_from_logits")
    SequenceSummaryStats = _ref(ref, "tianshou.data", "SequenceSummaryStats")
    PPO = _on_policy_base(algo, ref)

    from . import ppo_discrete as PD

    class HipPPODiscrete(_HipGlue, PPO):
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            actor, critic = self.policy.actor, self.critic
            sa, sc = actor.state_dict(), critic.state_dict()
            keys = PD.TRUNK_KEYS + PD.HEAD_KEYS
            if list(sa.keys()) != keys or list(sc.keys()) != keys or actor.preprocess is not critic.preprocess:
                raise NotImplementedError("HipPPODiscrete: actor / critic must share one Net(obs, [h, h]) trunk with "
                                          "single-Linear heads")
            hidden, n_act = sa[keys[0]].shape[0], sa[keys[4]].shape[0]
            if hidden % 32 or sa[keys[2]].shape != (hidden, hidden) or n_act > 31 or sc[keys[4]].shape[0] != 1:
                raise NotImplementedError("HipPPODiscrete: hidden sizes [h, h] with h a multiple of 32, <= 31 actions")
            # the actor's outputs must reach Categorical as what they are: probabilities or logits
            softmax = bool(getattr(actor, "softmax_output", True))
            dist_fn = self.policy.dist_fn
            if not ((softmax and dist_fn is Categorical) or (not softmax and dist_fn is dist_fn_categorical_from_logits)):
                raise NotImplementedError("HipPPODiscrete: softmax_output=True needs dist_fn=Categorical, "
                                          "softmax_output=False the logits dist_fn")
            optimizer_fields(self.optim._optim)                # Adam / RMSprop incl. weight decay (ts::optim_step)
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_params(self):
            return params_by_keys(self.policy.actor, PD.TRUNK_KEYS + PD.HEAD_KEYS) + params_by_keys(self.critic, PD.HEAD_KEYS)

        def _hip_parts(self, eng=None):
            params, dev = self._hip_params(), self._hip_device
            hidden, obs_dim = params[0].shape
            dims = (obs_dim, hidden, params[4].shape[0])
            return [_OnPart("params", ("adam_m", "adam_v"), self.optim, params,
                            lambda t: PD.flat_from_torch(t, *dims, dev), lambda f: PD.flat_to_torch(f, *dims))]

        def _engine(self):
            if self._hip_engine is None:
                part, = self._hip_parts()
                (hidden, obs_dim), n_act = part.params[0].shape, part.params[4].shape[0]
                self._hip_engine = _on_load(self, PD.DiscretePPOEngine(obs_dim, hidden, n_act, part.flat(), ppo_config_from(self)))
            return self._hip_engine

        _hip_write_back = _on_write_back

        def _hip_rewards(self, eng, m):
            """The rewards the returns are computed from, in sample_indices(0) order: None = the mirror's column, read in place
            (a reward-supplying wrapper -- HipICM -- leaves its float64 device tensor in `_hip_rew_source` for one call)."""
            return self.__dict__.get("_hip_rew_source")

        def _preprocess_batch(self, batch, buffer, indices):
            _require_gpu(self._hip_device, "HipPPODiscrete")
            eng = self._engine()
            m = _mirror(self, buffer, self._hip_device)
            rew = self._hip_rewards(eng, m)
            pre = self._hip_pre = eng.preprocess(m) if rew is None else eng.preprocess(m, rew=rew)
            batch.v_s, batch.returns, batch.adv, batch.logp_old = pre["v_s"], pre["returns"], pre["adv"], pre["logp_old"]
            return batch

        def _update_with_batch(self, batch, batch_size, repeat):
            self._hip_refresh_lr()
            eng, m = self._hip_engine, self._hip_mirror
            perms = [np.random.permutation(len(batch)) for _ in range(repeat)]     # Batch.split, batch.py:1209
            losses, steps = eng.update(m, self._hip_pre, batch_size, repeat, perms)
            self._hip_write_back()
            return _a2c_stats(A2CTrainingStats, SequenceSummaryStats.from_sequence, losses, steps)

    if algo == "a2c":
        HipPPODiscrete.__name__ = HipPPODiscrete.__qualname__ = "HipA2CDiscrete"
    return HipPPODiscrete


# ---------------------------------------------------------------------------------------------------
# ICM (modelbased/icm.py) around HipPPODiscrete / HipA2CDiscrete: the test/modelbased/test_ppo_icm.py pairing
# ---------------------------------------------------------------------------------------------------
def make_hip_icm(ref=None):
    """Returns HipICM(ICMOnPolicyWrapper) (icm.py:187-261) with the curiosity model on the engine (tianshou_amd/icm.py).
    `wrapped_algorithm` must be a HipPPODiscrete / HipA2CDiscrete; `model` an IntrinsicCuriosityModule whose feature net is a
    Linear / ReLU-or-tanh chain (`icm.describe_module` raises NotImplementedError naming anything else); Adam or RMSprop.
    `_preprocess_batch` gathers obs / act / obs_next from the wrapped algorithm's device mirror, adds float64(mse_loss *
    reward_scale) to the mirror's rewards (ts_icm_reward) and hands the result to the wrapped preprocessing, so GAE -- and PPO's
    recompute_advantage -- see the augmented rewards; `batch.rew` is that float64 DEVICE tensor until `_postprocess_batch`
    restores it.  `_wrapper_update_with_batch` runs the one optimizer step on the same rows (ts_icm_update) after the wrapped
    update and returns ICMTrainingStats from one read of the three statistics.  lr, lr_scale, reward_scale and
    forward_loss_weight are read at every update.  Actions outside [0, A) are clamped into it.
    `state_dict()` keeps the reference's keys.  `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    ICMOnPolicyWrapper = _ref(ref, "tianshou.algorithm.modelbased.icm", "ICMOnPolicyWrapper")
    ICMTrainingStats = _ref(ref, "tianshou.algorithm.modelbased.icm", "ICMTrainingStats")

    from . import icm as IC
    from .buffer import gather_rows

    class HipICM(_HipGlue, ICMOnPolicyWrapper):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            w = self.wrapped_algorithm
            if type(w).__name__ not in ("HipPPODiscrete", "HipA2CDiscrete") or not hasattr(w, "_hip_rewards"):
                raise NotImplementedError(f"HipICM: the wrapped algorithm must be a HipPPODiscrete or a HipA2CDiscrete "
                                          f"(found {type(w).__name__})")
            self._hip_device = w._hip_device
            self._hip_obs_dim = int(w._hip_params()[0].shape[1])
            d = IC.describe_module(self.model, self._hip_obs_dim)           # raises NotImplementedError naming what was found
            self._hip_icm = {k: v for k, v in d.items() if k != "tensors"}
            optimizer_fields(self.optim._optim)                             # (raises on an optimizer the engine does not implement)
            self._hip_rows = self._hip_orig_rew = None
            self._hip_engine = None
            self._hip_glue_init()

        # -- engine life cycle: the ICM model is this wrapper's own part; the wrapped algorithm keeps its engine ------------------
        def _hip_current_versions(self) -> tuple:
            # (the wrapped algorithm writes ITS parameters back after every update and watches them itself: only the model's count)
            return tuple((id(p), p._version) for p in self.model.parameters())

        def _hip_chain_dims(self):
            d = self._hip_icm
            return IC.chain_dims(self._hip_obs_dim, d["n_act"], d["feature_dim"], d["feat_hidden"], d["model_hidden"])

        def _hip_config(self):
            of = optimizer_fields(self.optim._optim)
            return IC.ICMConfig(lr_scale=float(self.lr_scale), reward_scale=float(self.reward_scale),
                                forward_loss_weight=float(self.forward_loss_weight), optimizer=of["optimizer"], lr=of["lr"],
                                betas=tuple(of.get("betas", (0.9, 0.999))), eps=of["adam_eps"], weight_decay=of["weight_decay"],
                                rms_alpha=of.get("rms_alpha", 0.99), rms_momentum=of.get("rms_momentum", 0.0),
                                rms_centered=of.get("rms_centered", False), max_grad_norm=self.optim._max_grad_norm)

        def _hip_parts(self, eng=None):
            dims, dev = self._hip_chain_dims(), self._hip_device
            params = IC.describe_module(self.model, self._hip_obs_dim)["tensors"]
            return [_OnPart("params", ("state_m", "state_v"), self.optim, params, lambda t: IC.flat_from_tensors(t, dims, dev),
                            lambda f: IC.flat_to_tensors(f, dims), step="optim_step")]

        def _engine(self):
            if self._hip_engine is None:
                d, (part,) = self._hip_icm, self._hip_parts()
                self._hip_engine = _on_load(self, IC.ICMEngine(self._hip_obs_dim, d["n_act"], d["feature_dim"], d["feat_hidden"],
                                                               d["feat_activation"], d["model_hidden"], part.flat(), self._hip_config()))
            return self._hip_engine

        def _hip_write_back(self) -> None:
            """After every update: the model's parameters.  Its optimizer moments are only needed by `state_dict()` and move there
            (`_hip_flush`), as HipPPO's do."""
            _on_write_back(self, optimizer=False)
            self._hip_adam_dirty = True

        def _hip_flush(self) -> None:
            if getattr(self, "_hip_adam_dirty", False):
                _on_write_back(self, params=False)
                self._hip_adam_dirty = False

        def load_state_dict(self, state_dict, *args, **kwargs):
            # nn.Module.state_dict calls the child's override, so the reference's checkpoint holds the wrapped algorithm's
            # optimizers under "wrapped_algorithm._optimizers" -- and Algorithm.load_state_dict (algorithm_base.py:533-543) pops
            # only its own key: the reference cannot load its own checkpoint with strict=True.  Here the nested entry goes where
            # it belongs, so a HipICM checkpoint (same keys) loads back strictly.
            state_dict = dict(state_dict)
            nested = state_dict.pop("wrapped_algorithm." + self._STATE_DICT_KEY_OPTIMIZERS, None)
            out = super().load_state_dict(state_dict, *args, **kwargs)
            if nested is not None:
                w = self.wrapped_algorithm
                for o, sd in zip(w._optimizers, nested):
                    o.load_state_dict(sd)
                w._hip_invalidate()
            return out

        def _hip_refresh_lr(self) -> None:
            super()._hip_refresh_lr()
            eng = self._hip_engine
            if eng is not None:                  # icm.py:73-75: plain attributes, read at every update like the learning rate
                eng.cfg.lr_scale, eng.cfg.reward_scale = float(self.lr_scale), float(self.reward_scale)
                eng.cfg.forward_loss_weight = float(self.forward_loss_weight)
                eng.cfg.max_grad_norm = self.optim._max_grad_norm

        # -- hooks ----------------------------------------------------------------------------------------------------------------
        def _preprocess_batch(self, batch, buffer, indices):
            """icm.py:236-243: the intrinsic reward with the model's current parameters, then the wrapped preprocessing."""
            _require_gpu(self._hip_device, "HipICM")
            w = self.wrapped_algorithm
            eng = self._engine()
            self._hip_refresh_lr()
            m = _mirror(w, buffer, self._hip_device)
            idx = m.sample_indices(0)
            rows = self._hip_rows = (gather_rows(m.obs, idx), m.act[idx].reshape(-1), m.obs_next_rows(idx))
            rew = eng.reward(*rows, m.rew[idx])
            self._hip_orig_rew = getattr(batch, "rew", None)
            w.__dict__["_hip_rew_source"] = rew              # the seam: HipPPODiscrete._hip_rewards
            try:
                batch = w._preprocess_batch(batch, buffer, indices)
            finally:
                w.__dict__["_hip_rew_source"] = None
            batch.rew = rew
            return batch

        def _postprocess_batch(self, batch, buffer, indices):
            """icm.py:245-252."""
            self.wrapped_algorithm._postprocess_batch(batch, buffer, indices)
            batch.rew = self._hip_orig_rew

        def _update_with_batch(self, batch, batch_size, repeat):
            # (defined here so that `_HipGlue` brackets it: the write-back below must not look like a foreign write)
            return super()._update_with_batch(batch, batch_size, repeat)

        def _wrapper_update_with_batch(self, batch, batch_size, repeat, original_stats):
            """icm.py:90-109, after the wrapped update, on the rows of `_preprocess_batch` (the model has not changed since)."""
            self._hip_refresh_lr()
            eng = self._engine()
            stats = eng.update(*self._hip_rows)
            self._hip_write_back()
            loss, fwd, inv = (float(x) for x in stats.cpu().numpy())         # the one read of the three statistics
            return ICMTrainingStats(original_stats, icm_loss=loss, icm_forward_loss=fwd, icm_inverse_loss=inv)

    return HipICM


# ---------------------------------------------------------------------------------------------------
# ICM around HipPPOCnn / HipA2CCnn: the examples/atari/atari_ppo.py:136-160 pairing (--icm-lr-scale)
# ---------------------------------------------------------------------------------------------------
def make_hip_icm_cnn(ref=None):
    """Returns HipICMCnn(ICMOnPolicyWrapper) with the curiosity model of atari_ppo.py on the engine (tianshou_amd/icm_cnn.py).
    `wrapped_algorithm` must be a HipPPOCnn / HipA2CCnn; `model` an IntrinsicCuriosityModule whose feature net is
    DQNet(c, h, w, action_shape, features_only=True).net (`icm_cnn.describe_module` raises NotImplementedError naming anything
    else); Adam or RMSprop.  The hooks are HipICM's (see `make_hip_icm`), over uint8 frames: `_preprocess_batch` walks
    sample_indices(0) chunk by chunk, gathering (and frame-stacking) obs and obs_next from the wrapped algorithm's mirror --
    obs_next from the stored column or, without one, obs at next(index) -- and hands the augmented float64 rewards to the
    wrapped preprocessing; `_wrapper_update_with_batch` gathers the same chunks again for the one optimizer step
    (ts_icm_cnn_grad per chunk, ts_icm_cnn_apply).  The frames of a rollout are never all resident as NHWC batches.
    Only the on-policy wrapper exists: the reference's off-policy n-step return reads buffer.rew, not batch.rew
    (algorithm_base.py:801-802), so ICMOffPolicyWrapper's intrinsic reward never reaches a target.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    ICMTrainingStats = _ref(ref, "tianshou.algorithm.modelbased.icm", "ICMTrainingStats")
    HipICM = make_hip_icm(ref)

    from . import icm_cnn as ICC
    from .dqn import gather_obs_nhwc

    class HipICMCnn(HipICM):
        def __init__(self, *args, **kwargs):
            super(HipICM, self).__init__(*args, **kwargs)                   # (HipICM's own checks are for the vector pairing)
            w = self.wrapped_algorithm
            if type(w).__name__ not in ("HipPPOCnn", "HipA2CCnn") or not hasattr(w, "_hip_rewards"):
                raise NotImplementedError(f"HipICMCnn: the wrapped algorithm must be a HipPPOCnn or a HipA2CCnn "
                                          f"(found {type(w).__name__})")
            self._hip_device = w._hip_device
            d = ICC.describe_module(self.model)           # raises NotImplementedError naming what was found; the frame size comes with the buffer
            self._hip_icm = {k: v for k, v in d.items() if k != "tensors"}
            optimizer_fields(self.optim._optim)
            self._hip_rows = self._hip_orig_rew = self._hip_frame = None
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_dims(self, eng=None):
            frame = (eng.c, eng.h, eng.w) if eng is not None else self._hip_frame
            if frame is None:
                raise RuntimeError("HipICMCnn: the frame size is known with the first buffer (no update has run yet)")
            return (*frame, self._hip_icm["n_act"], self._hip_icm["model_hidden"])

        def _hip_parts(self, eng=None):
            dims, dev = self._hip_dims(eng), self._hip_device
            params = ICC.describe_module(self.model, *dims[:3])["tensors"]
            return [_OnPart("params", ("state_m", "state_v"), self.optim, params, lambda t: ICC.flat_from_torch(t, *dims, dev),
                            lambda f: ICC.flat_to_torch(f, *dims), step="optim_step")]

        def _engine(self):
            if self._hip_engine is None:
                (part,), dims = self._hip_parts(), self._hip_dims()
                self._hip_engine = _on_load(self, ICC.ICMCnnEngine(*dims, part.flat(), self._hip_config()))
            return self._hip_engine

        def _hip_chunks(self, m, idx, stack):
            """rows(lo, hi) -> (obs, act, obs_next) of the transitions idx[lo:hi] as uint8 NHWC batches, gathered on demand."""
            act = m.act[idx].reshape(-1)

            def rows(lo, hi):
                i = idx[lo:hi]
                nxt = gather_obs_nhwc(m.obs_next, m, i, stack, as_u8=True) if m.obs_next is not None else \
                    gather_obs_nhwc(m.obs, m, m.next(i), stack, as_u8=True)         # buffer_base.py:622-626
                return gather_obs_nhwc(m.obs, m, i, stack, as_u8=True), act[lo:hi], nxt

            return rows

        def _preprocess_batch(self, batch, buffer, indices):
            """icm.py:236-243: the intrinsic reward with the model's current parameters, then the wrapped preprocessing."""
            _require_gpu(self._hip_device, "HipICMCnn")
            w = self.wrapped_algorithm
            c, h, wd, stack = w._layout(buffer)
            if self._hip_frame is not None and self._hip_frame != (c, h, wd):
                self._hip_engine = None                      # (another frame size: another layout)
            self._hip_frame = (c, h, wd)
            if c != self._hip_icm["c"]:
                raise NotImplementedError(f"HipICMCnn: the feature net takes {self._hip_icm['c']} channels, the buffer's frames have {c}")
            eng = self._engine()
            self._hip_refresh_lr()
            m = _mirror(w, buffer, self._hip_device)
            idx = m.sample_indices(0)
            n = idx.numel()
            rows = self._hip_rows = (self._hip_chunks(m, idx, stack), n)
            base = m.rew[idx]
            rew = torch.empty(n, dtype=torch.float64, device=self._hip_device)
            for lo in range(0, n, ICC.DEFAULT_CHUNK):
                hi = min(lo + ICC.DEFAULT_CHUNK, n)
                rew[lo:hi] = eng.reward(*rows[0](lo, hi), base[lo:hi])
            self._hip_orig_rew = getattr(batch, "rew", None)
            w.__dict__["_hip_rew_source"] = rew              # the seam: HipPPOCnn._hip_rewards
            try:
                batch = w._preprocess_batch(batch, buffer, indices)
            finally:
                w.__dict__["_hip_rew_source"] = None
            batch.rew = rew
            return batch

        def _wrapper_update_with_batch(self, batch, batch_size, repeat, original_stats):
            """icm.py:90-109, after the wrapped update, on the rows of `_preprocess_batch` (the model has not changed since)."""
            self._hip_refresh_lr()
            eng = self._engine()
            rows, n = self._hip_rows
            stats = eng.update(rows, n=n)
            self._hip_write_back()
            loss, fwd, inv = (float(x) for x in stats.cpu().numpy())         # the one read of the three statistics
            return ICMTrainingStats(original_stats, icm_loss=loss, icm_forward_loss=fwd, icm_inverse_loss=inv)

    return HipICMCnn


# ---------------------------------------------------------------------------------------------------
# TD3 / DDPG (td3.py:104-226, ddpg.py:343-411) on the mujoco_td3.py / mujoco_ddpg.py networks
# ---------------------------------------------------------------------------------------------------
def _make_hip_det(twin: bool, ref=None, bc: bool = False):
    """`bc`: TD3+BC (imitation/td3_bc.py), TD3 with the behaviour-cloning term in the actor loss -- the same hooks over
    tianshou_amd.td3bc.TD3BCEngine, with `alpha` read at every update."""
    DDPG = _ref(ref, "tianshou.algorithm.modelfree.ddpg", "DDPG")
    DDPGTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.ddpg", "DDPGTrainingStats")
    TD3 = _ref(ref, "tianshou.algorithm.modelfree.td3", "TD3")
    TD3TrainingStats = _ref(ref, "tianshou.algorithm.modelfree.td3", "TD3TrainingStats")

    from . import td3 as T

    base = TD3 if twin else DDPG
    if bc:
        from . import td3bc as TB

        base = _ref(ref, "tianshou.algorithm.imitation.td3_bc", "TD3BC")      # (OfflineAlgorithm first in its MRO)

    class HipDet(_HipGlue, base):
        _HIP_LR = (("actor_lr", "policy_optim"), ("critic_lr", "critic_optim")) + \
            ((("critic_lr", "critic2_optim"),) if twin else ())
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            nets = [("actor", self.policy.actor, T.actor_keys), ("critic1", self.critic, T.critic_keys)]
            keys = _ac_nets(self, "HipTD3 / HipDDPG", "networks must be those of examples/mujoco/mujoco_td3.py (Net trunks of "
                            "one depth, 1 .. 6 hidden layers, single-Linear action / Q heads)",
                            nets + ([("critic2", self.critic2, T.critic_keys)] if twin else []),
                            [self.policy_optim, self.critic_optim] + ([self.critic2_optim] if twin else []))
            self._hip_akeys, self._hip_ckeys = keys["actor"], keys["critic1"]
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_parts(self):
            o, a, h, dev, sz = self._hip_obs_dim, self._hip_act_dim, self._hip_hidden, self._hip_device, self._hip_sizes

            def part(name, mod, old, optim):
                # (the critics' step count is TD3's `_cnt`, which the algorithm keeps: `_engine` sets it, no optimizer is asked)
                actor = name == "actor"
                keys, fwd, back = ((self._hip_akeys, T.actor_flat_from_torch, T.actor_flat_to_torch) if actor else
                                   (self._hip_ckeys, T.critic_flat_from_torch, T.critic_flat_to_torch))
                return _ACPart(name, mod, old.module, optim, keys, lambda t: fwd(t, o, a, dev, hidden=h),
                               lambda f: back(f, o, a, h, sizes=sz[name]), "actor_steps" if actor else "cnt", actor)

            parts = [part("actor", self.policy.actor, self.actor_old, self.policy_optim),
                     part("critic1", self.critic, self.critic_old, self.critic_optim)]
            if twin:
                parts.append(part("critic2", self.critic2, self.critic2_old, self.critic2_optim))
            return parts

        def _engine(self):
            if self._hip_engine is None:
                Config, Engine = (TB.TD3BCConfig, TB.TD3BCEngine) if bc else (T.TD3Config, T.TD3Engine)
                cfg = Config(**_ac_config_fields(self), twin=twin,
                             policy_noise=getattr(self, "policy_noise", 0.0), noise_clip=getattr(self, "noise_clip", 0.0),
                             update_actor_freq=getattr(self, "update_actor_freq", 1),
                             max_action=float(self.policy.actor.max_action), **({"alpha": float(self.alpha)} if bc else {}))
                flats = {p.name: p.flat() for p in self._hip_parts()}
                eng = Engine(self._hip_obs_dim, self._hip_act_dim, flats["actor"], flats["critic1"], flats.get("critic2"), cfg,
                             hidden=self._hip_hidden, depth=self._hip_depth, activation=self._hip_actfn)
                eng.cnt = getattr(self, "_cnt", 0)
                self._hip_engine = _ac_load(self, eng)                               # resume from a checkpoint
            return self._hip_engine

        def _preprocess_batch(self, batch, buffer, indices):
            eng, m, idx = _ac_begin(self, "HipTD3 / HipDDPG", buffer, indices)
            noise = torch.randn(size=(len(indices), eng.act_dim)) if twin else None        # td3.py:196
            batch.returns = eng.preprocess(m, idx, noise).reshape(-1, 1)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            from .buffer import gather_rows_multi

            eng, m = self._hip_engine, self._hip_mirror
            if bc:
                eng.cfg.alpha = float(self.alpha)                                 # read at every update, as the learning rate
            stats, w = eng.update_with_batch(*gather_rows_multi([m.obs, m.act], self._hip_idx),
                                             batch.returns.reshape(-1), getattr(batch, "weight", None))
            batch.weight = w
            s = stats.cpu().numpy()
            self._cnt = eng.cnt                       # (DDPG has no `_cnt` of its own: kept for it too, a rebuilt engine starts from it)
            if twin:
                self._last = float(s[0])
            self._hip_after_update()
            if twin:
                return TD3TrainingStats(actor_loss=float(s[0]), critic1_loss=float(s[1]), critic2_loss=float(s[2]))
            return DDPGTrainingStats(actor_loss=float(s[0]), critic_loss=float(s[1]))

        _hip_write_back = _ac_write_back

    HipDet.__name__ = "HipTD3BC" if bc else "HipTD3" if twin else "HipDDPG"
    return HipDet


def make_hip_td3(ref=None):
    """Returns HipTD3(TD3) (hooks td3.py:190-226 on the engine).  `ref`: namespace replacing the tianshou imports."""
    return _make_hip_det(True, ref)


def make_hip_ddpg(ref=None):
    """Returns HipDDPG(DDPG) (hooks ddpg.py:397-411 on the engine)."""
    return _make_hip_det(False, ref)


def make_hip_td3bc(ref=None):
    """Returns HipTD3BC(TD3BC): TD3's hooks (td3.py:190-202, ddpg.py:287-301) with `_update_with_batch` of
    imitation/td3_bc.py:102-127 on the engine (tianshou_amd/td3bc.py).  Networks as HipTD3, always two critics (the reference
    copies critic 1 when it is given no second one).  The offline case is a plain ReplayBuffer / VectorReplayBuffer without
    `weight`; a prioritized buffer works as well.  `alpha` is read from the algorithm at every update; the statistics are
    TD3TrainingStats.  `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    return _make_hip_det(True, ref, bc=True)


# ---------------------------------------------------------------------------------------------------
# vanilla imitation learning / behaviour cloning (imitation/imitation_base.py)
# ---------------------------------------------------------------------------------------------------
class _BCRoute(NamedTuple):
    """What `make_hip_imitation` reads off the actor at construction."""
    kind: str             # "dqnet" | "discrete" | "continuous"
    keys: list            # state_dict keys of the actor in the converters' order
    n_out: int            # actions (discrete routes) or action dimensions
    obs_dim: int          # MLP routes (DQNet: 0, the frame shape comes with the first batch)
    sizes: tuple          # MLP routes: hidden widths of the torch network
    activation: str       # MLP routes: "relu" | "tanh"
    max_action: float     # continuous route


def _bc_route(policy, who: str) -> _BCRoute:
    """The engine route of an ImitationPolicy's actor, or NotImplementedError naming the actor's class: DQNet by its state_dict
    keys (as HipDQN), a Net with an action head (Linear / activation pairs and a final bare Linear), or a
    ContinuousActorDeterministic over a Net.  The action type must be the route's; activations nn.ReLU or nn.Tanh; no norm
    layer, softmax or dueling head; anything else (a recurrent model, a probabilistic actor) is refused, never run in eager."""
    from . import bc as BC
    from . import dqn as D
    from . import td3 as T
    from . import widths as WD

    actor = policy.actor
    name = type(actor).__name__
    action_type = getattr(policy, "action_type", None)
    keys = list(actor.state_dict().keys())

    def need(kind: str, want: str) -> None:
        if action_type != want:
            raise NotImplementedError(f"{who}: the {kind} route of actor {name} needs a {want} action space, the policy's action "
                                      f"type is {action_type!r}")

    if keys == D.TIANSHOU_KEYS:
        need("DQNet", "discrete")
        shapes = [tuple(p.shape) for p in params_by_keys(actor, keys)]
        if not (len(shapes[0]) == 4 and shapes[0][0] == 32 and shapes[0][2:] == (8, 8) and shapes[2] == (64, 32, 4, 4)
                and shapes[4] == (64, 64, 3, 3) and shapes[6][0] == 512):
            raise NotImplementedError(f"{who}: unsupported actor {name}: not the DQNet(c, h, w, action_shape) convolution trunk")
        n_act = int(shapes[8][0])
        if not 1 <= n_act <= BC.MAX_ACT:
            raise NotImplementedError(f"{who}: actor {name}: 1 .. {BC.MAX_ACT} actions, got {n_act}")
        return _BCRoute("dqnet", keys, n_act, 0, (), "relu", 0.0)
    # ContinuousActorDeterministic over a Net (`head`), or Net(state_shape, action_shape, hidden_sizes) itself
    head = hasattr(actor, "preprocess") and hasattr(actor, "last") and hasattr(actor, "max_action")
    seq = getattr(getattr(actor.preprocess if head else actor, "model", None), "model", None)
    seq = list(seq) if isinstance(seq, torch.nn.Sequential) else None
    if seq is None:
        raise NotImplementedError(f"{who}: unsupported actor {name}: DQNet, Net(state_shape, action_shape, hidden_sizes) or "
                                  "ContinuousActorDeterministic over a Net (a recurrent or probabilistic actor has no engine route)")
    norms = [type(m).__name__ for m in seq if "Norm" in type(m).__name__]
    if norms:
        raise NotImplementedError(f"{who}: actor {name} has a norm layer ({norms[0]}); the engine's trunks have none")
    body = seq if head else seq[:-1]
    acts = {type(m) for m in body[1::2]}
    pairs_ok = len(body) >= 2 and len(body) % 2 == 0 and all(isinstance(m, torch.nn.Linear) for m in body[0::2])
    if not pairs_ok or (not head and not isinstance(seq[-1], torch.nn.Linear)):
        raise NotImplementedError(f"{who}: unsupported actor {name}: the trunk must be Linear layers, each followed by its "
                                  f"activation (got {[type(m).__name__ for m in seq]})")
    if len(acts) != 1 or next(iter(acts)) not in (torch.nn.ReLU, torch.nn.Tanh):
        raise NotImplementedError(f"{who}: actor {name}: activation nn.ReLU or nn.Tanh after every hidden layer, got "
                                  f"{sorted(a.__name__ for a in acts)}")
    activation = "relu" if next(iter(acts)) is torch.nn.ReLU else "tanh"
    depth = len(body) // 2
    if not 1 <= depth <= WD.MAX_DEPTH:
        raise NotImplementedError(f"{who}: actor {name}: 1 .. {WD.MAX_DEPTH} hidden layers, got {depth}")
    if head:
        if keys != T.actor_keys(depth):
            raise NotImplementedError(f"{who}: unsupported actor {name}: a Net trunk and a single-Linear action head are needed "
                                      f"(got parameters {keys})")
        need("continuous MLP", "continuous")
    else:
        if keys != [f"model.model.{2 * i}.{x}" for i in range(depth + 1) for x in ("weight", "bias")] \
                or getattr(actor, "softmax", False) or getattr(actor, "use_dueling", False):
            raise NotImplementedError(f"{who}: unsupported actor {name}: Net(state_shape, action_shape, hidden_sizes) without "
                                      "softmax or dueling heads is needed")
        need("discrete MLP", "discrete")
    t = [p.detach() for p in params_by_keys(actor, keys)]
    try:
        sizes = WD.layer_widths(t, 1)
        WD.engine_hidden([sizes])
    except NotImplementedError as e:
        raise NotImplementedError(f"{who}: actor {name}: hidden layers of widths up to 1024 ({e})") from None
    n_out = int(t[-1].shape[0])
    lo, hi = (1, BC.MAX_ACT_DIM) if head else (2, BC.MAX_ACT)
    if not lo <= n_out <= hi:
        raise NotImplementedError(f"{who}: actor {name}: the MLP head holds {lo} .. {hi} outputs, got {n_out}")
    return _BCRoute("continuous" if head else "discrete", keys, n_out, int(t[0].shape[1]), tuple(sizes), activation,
                    float(actor.max_action) if head else 0.0)


def make_hip_imitation(offline: bool, ref=None):
    """Returns HipOfflineImitationLearning(OfflineImitationLearning) (`offline=True`) or
    HipOffPolicyImitationLearning(OffPolicyImitationLearning): `_update_with_batch` (imitation/imitation_base.py:109-127, 151-155,
    179-183) on the engines of tianshou_amd/bc.py.  The route is chosen from `policy.actor` at construction (`_bc_route`): DQNet
    on u8 / f32 frames, Net with an action head, ContinuousActorDeterministic over a Net; everything else raises
    NotImplementedError, as does an optimizer other than Adam.  `_preprocess_batch` stays the base class's: the batch's `obs` and
    `act` are what the buffer sampled ([B, c, h, w] frames are laid out NHWC on the device, as the other Atari classes' gathers
    do).  The collector's `policy.forward` stays on torch; `action_scaling` / `action_bound_method` act in `map_action` only
    and are not read.  The statistics are the reference's ImitationTrainingStats(loss).  `write_back`: as HipDQN.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    from . import bc as BC
    from . import dqn as D

    mod = "tianshou.algorithm.imitation.imitation_base"
    Base = _ref(ref, mod, "OfflineImitationLearning" if offline else "OffPolicyImitationLearning")
    ImitationTrainingStats = _ref(ref, mod, "ImitationTrainingStats")
    who = "HipOfflineImitationLearning" if offline else "HipOffPolicyImitationLearning"

    class HipImitation(_HipGlue, Base):
        def __init__(self, *args, device="cuda", write_back="auto", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            self._hip_route = _bc_route(self.policy, who)
            try:
                _adam_of(self.optim)
            except NotImplementedError as e:
                raise NotImplementedError(f"{who}: {e} (got {type(self.optim._optim).__name__})") from None
            own = {id(p) for p in self.policy.actor.parameters()}
            if {id(p) for g in self.optim._optim.param_groups for p in g["params"]} != own:
                raise NotImplementedError(f"{who}: one optimizer over the actor's parameters")
            self._hip_chw = None
            self._hip_engine = None
            self._hip_glue_init()
            self._hip_set_write_back(write_back, attached=False)

        def _hip_parts(self, eng=None):
            r, dev = self._hip_route, self._hip_device
            params = params_by_keys(self.policy.actor, r.keys)
            if r.kind == "dqnet":
                dims = (*self._hip_chw, r.n_out)
                fwd, back = (lambda t: D.flat_from_torch(t, *dims, dev)), (lambda f: D.flat_to_torch(f, *dims))
            else:
                h = self._hip_hidden
                fwd = lambda t: BC.mlp_flat_from_torch(r.kind, t, r.obs_dim, r.n_out, h, dev)          # noqa: E731
                back = lambda f: BC.mlp_flat_to_torch(r.kind, f, r.obs_dim, r.n_out, h, sizes=r.sizes)  # noqa: E731
            return [_OnPart("params", ("adam_m", "adam_v"), self.optim, params, fwd, back)]

        def _hip_config(self):
            _, g = _adam_of(self.optim)
            return BC.BCConfig(lr=g["lr"], betas=tuple(g["betas"]), adam_eps=g["eps"], max_grad_norm=self.optim._max_grad_norm,
                               max_action=self._hip_route.max_action or 1.0)

        def _engine(self, obs_shape):
            r = self._hip_route
            if r.kind == "dqnet":
                if len(obs_shape) != 4 or obs_shape[1] != params_by_keys(self.policy.actor, r.keys)[0].shape[1]:
                    raise NotImplementedError(f"{who}: DQNet observations must be [B, c, h, w] frames, got {tuple(obs_shape)}")
                chw = tuple(int(x) for x in obs_shape[1:])
                if self._hip_engine is not None and chw != self._hip_chw:
                    raise ValueError(f"{who}: the frame shape changed from {self._hip_chw} to {chw}")
                self._hip_chw = chw
            if self._hip_engine is None:
                if r.kind == "dqnet":
                    eng = BC.BCDQNetEngine(*self._hip_chw, r.n_out, self._hip_parts()[0].flat(), self._hip_config())
                else:
                    from . import widths as WD

                    self._hip_hidden = WD.engine_hidden([r.sizes])
                    eng = BC.BCMlpEngine(r.kind, r.obs_dim, r.n_out, self._hip_parts()[0].flat(), self._hip_config(),
                                         hidden=self._hip_hidden, depth=len(r.sizes), activation=r.activation)
                self._hip_engine = _on_load(self, eng)                               # resume from a checkpoint
            return self._hip_engine

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            _require_gpu(self._hip_device, who)
            r, dev = self._hip_route, self._hip_device
            obs = batch.obs if isinstance(batch.obs, torch.Tensor) else torch.as_tensor(np.asarray(batch.obs))
            eng = self._engine(obs.shape)
            eng.cfg.max_grad_norm = self.optim._max_grad_norm              # read at every update, as the learning rate
            obs = obs.to(dev)
            if r.kind == "dqnet":
                if obs.dtype not in (torch.uint8, torch.float32):
                    obs = obs.to(torch.float32)
                obs = obs.permute(0, 2, 3, 1).contiguous()                  # [B, c, h, w] -> NHWC, dtype kept (u8 frames stay u8)
            else:
                obs = obs.reshape(obs.shape[0], -1)
            act = batch.act if isinstance(batch.act, torch.Tensor) else torch.as_tensor(np.asarray(batch.act))
            loss = eng.update_with_batch(obs, act.to(dev))
            self._hip_after_update()
            return ImitationTrainingStats(loss=float(loss.item()))                    # imitation_base.py:127

        _hip_write_back = _on_write_back

    HipImitation.__name__ = HipImitation.__qualname__ = who
    return HipImitation


# ---------------------------------------------------------------------------------------------------
# continuous CQL (imitation/cql.py) on the nets of examples/offline/d4rl_cql.py
# ---------------------------------------------------------------------------------------------------
def make_hip_cql(ref=None):
    """Returns HipCQL(CQL): `_update_with_batch` of imitation/cql.py:268-400 on the engine (tianshou_amd/cql.py over
    ts_cql_update).  Networks as HipSAC's (Net trunks of one depth, single-Linear mu / sigma / Q heads), Adam on the three
    optimizers, a fixed alpha or AutoAlpha.  `_preprocess_batch` only takes the device mirror of the buffer and the indices;
    `_update_with_batch` gathers the rows on the device: obs, act, rew, obs_next and `done` from the mirror,
    `calibration_returns` (calibrated=True; `process_buffer` stays the reference's and adds it to the buffer once) from a column
    uploaded once per mirror.  The five random tensors of an update are drawn from torch's default generator in the reference's
    order and calls (`update_noise="torch"`: randn [B, A] twice, `FloatTensor(B R, A).uniform_(-min_action, max_action)`, randn
    [B R, A] twice -- with the defaults min_action = -1, max_action = 1 that is uniform_(1, 1), every random action 1.0, as in the
    reference) or from the engine's Philox stream (`"device"`, the default, keyed as in HipSAC).  `cql_weight`, `temperature`,
    `lagrange_threshold` and the learning rates are read from the algorithm at every update.
    The Lagrange multiplier LEARNS, as in the reference on the CPU; on a cuda device the reference's `cql_log_alpha.to(device)`
    is a copy its optimizer never steps.  The write-back stores `cql_log_alpha` and `cql_alpha_optim`'s Adam state (step = the
    number of updates); since the reference keeps neither in `state_dict()`, HipCQL adds them under `_hip_cql_alpha` and loads
    them from there, so a checkpoint resumes.  The collector's `policy.forward` stays the reference's.
    `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    CQL = _ref(ref, "tianshou.algorithm.imitation.cql", "CQL")
    CQLTrainingStats = _ref(ref, "tianshou.algorithm.imitation.cql", "CQLTrainingStats")
    AutoAlpha = _ref(ref, "tianshou.algorithm.modelfree.sac", "AutoAlpha")

    from . import cql as Q
    from . import sac as S

    class HipCQL(_HipGlue, CQL):
        _HIP_LR = (("actor_lr", "policy_optim"), ("critic_lr", "critic_optim"), ("critic_lr", "critic2_optim"),
                   ("alpha_lr", "alpha"), ("cql_alpha_lr", "cql_alpha_optim"))
        _HIP_STATE_KEY = "_hip_cql_alpha"

        def __init__(self, *args, device="cuda", update_noise="device", noise_seed=None, **kwargs):
            super().__init__(*args, **kwargs)
            if update_noise not in ("device", "torch"):
                raise ValueError("update_noise must be 'device' or 'torch'")
            self._hip_update_noise, self._hip_noise_calls = update_noise, 0
            self._hip_noise_key = int(torch.initial_seed() % (2**31 - 1)) if noise_seed is None else int(noise_seed)
            self._hip_device = torch.device(device)
            keys = _ac_nets(self, "HipCQL", "networks must be those of examples/offline/d4rl_cql.py (Net trunks of one depth, "
                            "1 .. 6 hidden layers, single-Linear mu / sigma / Q heads)",
                            (("actor", self.policy.actor, S.actor_keys), ("critic1", self.critic, S.critic_keys),
                             ("critic2", self.critic2, S.critic_keys)), (self.policy_optim, self.critic_optim, self.critic2_optim))
            self._hip_akeys, self._hip_ckeys = keys["actor"], keys["critic1"]
            self._hip_bound = _actor_bound(self.policy.actor)
            g = self.cql_alpha_optim.param_groups[0]
            if type(self.cql_alpha_optim).__name__ != "Adam" or tuple(g["betas"]) != (0.9, 0.999) or g["eps"] != 1e-8:
                raise NotImplementedError("HipCQL: cql_alpha_optim must be torch.optim.Adam with its default betas / eps")
            self._hip_engine = None
            self._hip_glue_init()

        def hip_extra_state(self) -> dict:
            return {"update_noise_calls": int(self._hip_noise_calls)}

        def load_hip_extra_state(self, state: dict) -> None:
            if "update_noise_calls" in state:
                self._hip_noise_calls = int(state["update_noise_calls"])

        def _hip_cql_leaf(self):
            """The tensor `cql_alpha_optim` steps (cql.py:188-191: `self.cql_log_alpha` itself on the CPU, its source on cuda)."""
            return self.cql_alpha_optim.param_groups[0]["params"][0]

        def _hip_cql_fields(self) -> dict:
            mg = self.critic_optim._max_grad_norm
            return dict(cql_alpha_lr=float(self.cql_alpha_optim.param_groups[0]["lr"]), cql_weight=float(self.cql_weight),
                        temperature=float(self.temperature), with_lagrange=bool(self.with_lagrange),
                        lagrange_threshold=float(self.lagrange_threshold), min_action=float(self.min_action),
                        max_action=float(self.max_action), num_repeat_actions=int(self.num_repeat_actions),
                        alpha_min=float(self.alpha_min), alpha_max=float(self.alpha_max), max_grad_norm=0.0 if mg is None else float(mg),
                        calibrated=bool(self.calibrated))

        def _engine(self):
            if self._hip_engine is None:
                ga, gc = _adam_of(self.policy_optim)[1], _adam_of(self.critic_optim)[1]
                flats = {p.name: p.flat() for p in self._hip_parts()}
                cfg = Q.CQLConfig(gamma=self.gamma, tau=self.tau, actor_lr=ga["lr"], critic_lr=gc["lr"], betas=tuple(ga["betas"]),
                                  adam_eps=ga["eps"], **_ac_entropy_fields(self, AutoAlpha), **self._hip_cql_fields())
                eng = Q.CQLEngine(self._hip_obs_dim, self._hip_act_dim, flats["actor"], flats["critic1"], flats["critic2"], cfg,
                                  hidden=self._hip_hidden, depth=self._hip_depth, max_action=self._hip_bound, activation=self._hip_actfn)
                eng = _ac_load(self, eng)                      # resume: lagged critics, Adam moments / steps of a loaded checkpoint
                leaf = self._hip_cql_leaf()
                eng.cql_log_alpha[0] = float(leaf.detach().reshape(-1)[0])
                st = self.cql_alpha_optim.state.get(leaf, {})
                if "exp_avg" in st:
                    eng.cql_log_alpha_m[0], eng.cql_log_alpha_v[0] = float(st["exp_avg"]), float(st["exp_avg_sq"])
                    eng.adam_step = max(eng.adam_step, int(float(st["step"])))
                self._hip_engine = eng
            return self._hip_engine

        def _hip_parts(self):
            o, a, h, dev, sz = self._hip_obs_dim, self._hip_act_dim, self._hip_hidden, self._hip_device, self._hip_sizes

            def part(name, mod, old, optim, keys, fwd, back):
                return _ACPart(name, mod, old, optim, keys, lambda t: fwd(t, o, a, dev, hidden=h),
                               lambda f: back(f, o, a, h, sizes=sz[name]), "adam_step", True)

            return (part("actor", self.policy.actor, None, self.policy_optim, self._hip_akeys, S.actor_flat_from_torch, S.actor_flat_to_torch),
                    part("critic1", self.critic, self.critic_old.module, self.critic_optim, self._hip_ckeys,
                         S.critic_flat_from_torch, S.critic_flat_to_torch),
                    part("critic2", self.critic2, self.critic2_old.module, self.critic2_optim, self._hip_ckeys,
                         S.critic_flat_from_torch, S.critic_flat_to_torch))

        def _preprocess_batch(self, batch, buffer, indices):
            _ac_begin(self, "HipCQL", buffer, indices)         # the mirror and the indices; the rows are gathered on the device
            return batch

        def _hip_calibration_column(self, buffer, m):
            """`calibration_returns` of the buffer (cql.py:244-266) as a float32 device column, uploaded once per mirror."""
            have = self.__dict__.get("_hip_calib")
            if have is None or have[0] is not m:
                col = getattr(buffer._meta, "calibration_returns", None)
                if col is None:
                    raise RuntimeError("HipCQL: calibrated=True needs `calibration_returns` in the buffer (call process_buffer first)")
                have = self.__dict__["_hip_calib"] = (m, torch.as_tensor(np.asarray(col, np.float32), device=self._hip_device))
            return have[1]

        def _hip_noises(self, b: int, r: int, a: int):
            """The five random tensors of one update, in the reference's draw order."""
            if self._hip_update_noise == "torch":
                n1, n2 = torch.randn(b, a), torch.randn(b, a)
                ra = torch.FloatTensor(b * r, a).uniform_(-self.min_action, self.max_action)          # cql.py:303-307
                return n1, n2, ra, torch.randn(b * r, a), torch.randn(b * r, a)
            from .buffer import normal_noise

            key, c = self._hip_noise_key ^ 0xC91, self._hip_noise_calls
            self._hip_noise_calls += 5
            dev = self._hip_device
            n = [normal_noise(s, key, c + i, dev) for i, s in enumerate(((b, a), (b, a), (b * r, a), (b * r, a), (b * r, a)), 1)]
            # uniform_(lo, hi) from the third stream: Phi(z) is uniform on (0, 1)
            lo, hi = -float(self.min_action), float(self.max_action)
            ra = lo + (hi - lo) * (0.5 * (1.0 + torch.erf(n[2] * 0.7071067811865476)))
            return n[0], n[1], ra, n[3], n[4]

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            from .buffer import gather_rows_multi

            eng, m, idx = self._hip_engine, self._hip_mirror, self._hip_idx
            for k, v in self._hip_cql_fields().items():          # read at every update, as the learning rates
                if k in ("num_repeat_actions", "calibrated", "with_lagrange") and getattr(eng.cfg, k) != v:
                    raise NotImplementedError(f"HipCQL: `{k}` changed after the engine was built (call hip_invalidate())")
                setattr(eng.cfg, k, v)
            obs, act, obs_next = gather_rows_multi([m.obs, m.act, m.obs_next], idx)
            rew, done = m.rew[idx].to(torch.float32), m.done[idx].to(torch.float32)
            calib = self._hip_calibration_column(self._hip_mirror_src, m)[idx] if eng.cfg.calibrated else None
            b = int(idx.numel())
            stats = eng.update_with_batch(obs, act, rew, done, obs_next, *self._hip_noises(b, eng.cfg.num_repeat_actions, eng.act_dim),
                                          calib=calib)
            s = stats.cpu().numpy()                                               # one D2H per update()
            self._hip_after_update()
            auto, lag = eng.cfg.auto_alpha, eng.cfg.with_lagrange
            return CQLTrainingStats(actor_loss=float(s[0]), critic1_loss=float(s[1]), critic2_loss=float(s[2]), alpha=float(s[3]),
                                    alpha_loss=float(s[4]) if auto else None, cql_alpha_loss=float(s[6]) if lag else None,
                                    cql_alpha=float(s[5]) if lag else None)

        def _hip_write_back(self) -> None:
            _ac_write_back(self)
            eng = self.__dict__.get("_hip_engine_obj")
            if eng is None or not eng.cfg.with_lagrange:
                return
            leaf = self._hip_cql_leaf()
            with torch.no_grad():
                leaf.copy_(eng.cql_log_alpha.reshape(leaf.shape))
                if self.cql_log_alpha is not leaf:
                    self.cql_log_alpha.copy_(eng.cql_log_alpha.reshape(self.cql_log_alpha.shape))
            if eng.adam_step:
                store_adam_state(self.cql_alpha_optim, [leaf], [eng.cql_log_alpha_m], [eng.cql_log_alpha_v], eng.adam_step)

        def state_dict(self, *args, **kwargs):
            d = super().state_dict(*args, **kwargs)
            d[self._HIP_STATE_KEY] = {"cql_log_alpha": self._hip_cql_leaf().detach().clone(), "optim": self.cql_alpha_optim.state_dict()}
            return d

        def load_state_dict(self, state_dict, *args, **kwargs):
            state_dict = dict(state_dict)
            extra = state_dict.pop(self._HIP_STATE_KEY, None)
            out = super().load_state_dict(state_dict, *args, **kwargs)
            if extra is not None:
                leaf = self._hip_cql_leaf()
                with torch.no_grad():
                    leaf.copy_(extra["cql_log_alpha"].reshape(leaf.shape))
                    if self.cql_log_alpha is not leaf:
                        self.cql_log_alpha.copy_(extra["cql_log_alpha"].reshape(self.cql_log_alpha.shape))
                self.cql_alpha_optim.load_state_dict(extra["optim"])
                self._hip_invalidate()
            return out

    return HipCQL


# ---------------------------------------------------------------------------------------------------
# continuous BCQ (imitation/bcq.py) on the nets of examples/offline/d4rl_bcq.py
# ---------------------------------------------------------------------------------------------------
def _mlp_linears(net, who: str, what: str, output: bool):
    """The Linear layers of an `MLP` (`.model` is the nn.Sequential) or of a `Net` around one (`.model.model`): Linear, activation,
    ... with nn.ReLU or nn.Tanh after every hidden Linear and, with `output`, one last Linear without.  -> (hidden Linears + the
    output Linear, "relu" | "tanh")."""
    seq = getattr(net, "model", None)
    seq = getattr(seq, "model", seq)
    ms = list(seq) if isinstance(seq, torch.nn.Sequential) else []
    body = ms[:-1] if output else ms
    ok = len(body) >= 2 and len(body) % 2 == 0 and (not output or type(ms[-1]) is torch.nn.Linear) and all(
        type(body[i]) is torch.nn.Linear and type(body[i + 1]) in (torch.nn.ReLU, torch.nn.Tanh) for i in range(0, len(body), 2))
    acts = {type(body[i]) for i in range(1, len(body), 2)} if ok else set()
    if not ok or len(acts) != 1:
        raise NotImplementedError(f"{who}: {what} must be an MLP / Net trunk of 1 .. 6 hidden Linear layers with one activation class "
                                  f"(nn.ReLU or nn.Tanh) after each{' and a single Linear output layer' if output else ''} "
                                  f"(got {[type(m).__name__ for m in ms]})")
    return [m for m in ms if type(m) is torch.nn.Linear], "relu" if acts.pop() is torch.nn.ReLU else "tanh"


def make_hip_bcq(ref=None):
    """Returns HipBCQ(BCQ): `_update_with_batch` of imitation/bcq.py:188-263 on the engine (tianshou_amd/cbcq.py over
    ts_cbcq_update).  Supported networks, those of examples/offline/d4rl_bcq.py: `Perturbation` over an `MLP` or a `Net` with an
    action-sized output layer, two `ContinuousCritic(Net(concat=True))` with a single-Linear head, and a `VAE` whose encoder and
    decoder are `MLP`s; every trunk 1 .. 6 hidden layers with nn.ReLU or nn.Tanh, one depth and activation for the perturbation
    net and the critics, one for encoder and decoder; Adam with the same betas / eps on the four optimizers.
    `Perturbation.forward` takes `[0]` of its preprocess net's output (continuous.py:409): of the (logits, state) pair of a `Net`,
    but the first ROW of the logits of a plain `MLP` (the example's choice), so that every row of a batch is perturbed by the first
    row's logits.  HipBCQ computes what the reference computes in either case (`cfg.pert_first_row`).
    `_preprocess_batch` only takes the device mirror of the buffer and the indices; `_update_with_batch` gathers obs, act, rew,
    `done` and obs_next on the device.  The three normal draws of an update come from torch's default generator in the reference's
    order and shapes (`update_noise="torch"`: randn [B, L], [B R, L], [B, L]) or from the engine's Philox stream (`"device"`, the
    default).  The learning rates, `lmbda`, `gamma`, `tau` and `phi` are read from the algorithm at every update; a changed
    `num_sampled_action` or `latent_dim` raises (call `hip_invalidate()`).  Write-back and the `state_dict` round trip cover the
    four networks, the three lagged copies (`actor_perturbation_target` is kept up to date although nothing reads it, as in the
    reference) and the four Adam states.  The collector's `policy.forward` stays the reference's Python loop (HipPPO's
    `policy_forward="hip"` hook is written for its Gaussian policies); `hip_policy_forward(obs)` is the engine's forward for all
    observations at once.  `ref`: optional namespace replacing the tianshou imports (see `_ref`)."""
    BCQ = _ref(ref, "tianshou.algorithm.imitation.bcq", "BCQ")
    BCQTrainingStats = _ref(ref, "tianshou.algorithm.imitation.bcq", "BCQTrainingStats")

    from . import cbcq as Q
    from . import widths as WD

    who = "HipBCQ"

    class HipBCQ(_HipGlue, BCQ):
        _HIP_LR = (("pert_lr", "actor_perturbation_optim"), ("critic1_lr", "critic_optim"), ("critic2_lr", "critic2_optim"),
                   ("vae_lr", "vae_optim"))

        def __init__(self, *args, device="cuda", update_noise="device", noise_seed=None, **kwargs):
            super().__init__(*args, **kwargs)
            if update_noise not in ("device", "torch"):
                raise ValueError("update_noise must be 'device' or 'torch'")
            self._hip_update_noise, self._hip_noise_calls = update_noise, 0
            self._hip_noise_key = int(torch.initial_seed() % (2**31 - 1)) if noise_seed is None else int(noise_seed)
            self._hip_device = torch.device(device)
            pol = self.policy
            pert, vae = pol.actor_perturbation, pol.vae
            # an `MLP` (`.model` is the Sequential) returns the logits, a `Net` (`.model` is an MLP) a (logits, state) pair
            self._hip_first_row = isinstance(getattr(pert.preprocess_net, "model", None), torch.nn.Sequential)
            lp, act_p = _mlp_linears(pert.preprocess_net, who, "the perturbation net", True)
            trunks = [(lp, act_p)]
            for c in (pol.critic, self.critic2):
                lc, act_c = _mlp_linears(getattr(c, "preprocess", None), who, "a critic's preprocess net", False)
                head = list(getattr(getattr(c, "last", None), "model", []))
                if len(head) != 1 or type(head[0]) is not torch.nn.Linear or head[0].out_features != 1:
                    raise NotImplementedError(f"{who}: a critic's head must be a single Linear layer with one output")
                trunks.append((lc + head, act_c))
            le, act_e = _mlp_linears(vae.encoder, who, "the VAE's encoder", False)
            ld, act_d = _mlp_linears(vae.decoder, who, "the VAE's decoder", True)
            if type(vae.mean) is not torch.nn.Linear or type(vae.log_std) is not torch.nn.Linear:
                raise NotImplementedError(f"{who}: the VAE's mean / log_std heads must be single Linear layers")
            if len({len(t[0]) for t in trunks}) != 1 or len({t[1] for t in trunks}) != 1 or len(le) + 1 != len(ld) or act_e != act_d:
                raise NotImplementedError(f"{who}: one depth and one activation for the perturbation net and the critics, and one "
                                          "for the VAE's encoder and decoder")
            self._hip_depth, self._hip_actfn, self._hip_vdepth, self._hip_vactfn = len(lp) - 1, act_p, len(le), act_e
            if not 1 <= self._hip_depth <= WD.MAX_DEPTH or not 1 <= self._hip_vdepth <= WD.MAX_DEPTH:
                raise NotImplementedError(f"{who}: 1 .. {WD.MAX_DEPTH} hidden layers per trunk")
            self._hip_act_dim, self._hip_latent = int(lp[-1].out_features), int(vae.mean.out_features)
            self._hip_obs_dim = int(lp[0].in_features) - self._hip_act_dim
            if ld[0].in_features != self._hip_obs_dim + self._hip_latent or ld[-1].out_features != self._hip_act_dim \
                    or not 1 <= self._hip_latent <= 64 or self._hip_act_dim > 32:
                raise NotImplementedError(f"{who}: decoder on concat(obs, z) with act_dim <= 32 outputs, latent_dim in [1, 64]")
            wd = lambda ls: tuple(int(m.out_features) for m in ls)  # noqa: E731
            self._hip_sizes = {"pert": wd(lp[:-1]), "critic1": wd(trunks[1][0][:-1]), "critic2": wd(trunks[2][0][:-1]),
                               "enc": wd(le), "dec": wd(ld[:-1])}
            try:
                self._hip_hidden = WD.engine_hidden([self._hip_sizes[n] for n in ("pert", "critic1", "critic2")])
                self._hip_vhidden = WD.engine_hidden([self._hip_sizes["enc"], self._hip_sizes["dec"]])
            except NotImplementedError as e:
                raise NotImplementedError(f"{who}: hidden layers of widths up to 1024 per network ({e})") from None
            groups = [_adam_of(o)[1] for o in (self.actor_perturbation_optim, self.critic_optim, self.critic2_optim, self.vae_optim)]
            if len({(tuple(g["betas"]), g["eps"]) for g in groups}) != 1:
                raise NotImplementedError(f"{who}: one (betas, eps) for the four Adam optimizers")
            self._hip_keys = {"pert": list(pert.state_dict().keys()), "critic1": list(pol.critic.state_dict().keys()),
                              "critic2": list(self.critic2.state_dict().keys()), "vae": list(vae.state_dict().keys())}
            self._hip_engine = None
            self._hip_glue_init()

        def hip_extra_state(self) -> dict:
            return {"update_noise_calls": int(self._hip_noise_calls)}

        def load_hip_extra_state(self, state: dict) -> None:
            if "update_noise_calls" in state:
                self._hip_noise_calls = int(state["update_noise_calls"])

        def _hip_cbcq_fields(self) -> dict:
            pert = self.policy.actor_perturbation
            norm = lambda o: 0.0 if o._max_grad_norm is None else float(o._max_grad_norm)  # noqa: E731
            g = _adam_of(self.vae_optim)[1]
            lr = lambda o: float(_adam_of(o)[1]["lr"])  # noqa: E731
            return dict(gamma=float(self.gamma), tau=float(self.tau), lmbda=float(self.lmbda), phi=float(pert.phi),
                        max_action=float(pert.max_action), num_sampled_action=int(self.num_sampled_action),
                        forward_sampled_times=int(self.policy.forward_sampled_times), pert_lr=lr(self.actor_perturbation_optim),
                        critic1_lr=lr(self.critic_optim), critic2_lr=lr(self.critic2_optim), vae_lr=lr(self.vae_optim),
                        betas=tuple(g["betas"]), adam_eps=float(g["eps"]), pert_max_grad_norm=norm(self.actor_perturbation_optim),
                        critic1_max_grad_norm=norm(self.critic_optim), critic2_max_grad_norm=norm(self.critic2_optim),
                        vae_max_grad_norm=norm(self.vae_optim), pert_first_row=self._hip_first_row)

        def _hip_parts(self):
            o, a, ld, dev, sz = self._hip_obs_dim, self._hip_act_dim, self._hip_latent, self._hip_device, self._hip_sizes
            h, d, hv, dv = self._hip_hidden, self._hip_depth, self._hip_vhidden, self._hip_vdepth
            ne = 2 * dv + 4                                  # encoder trunk + mean + log_std tensors in the VAE's state_dict order
            k = self._hip_keys

            def vae_to(f):
                enc, dec = Q.vae_flat_to_torch(f, o, a, ld, hv, dv, sz["enc"], sz["dec"])
                return enc + dec

            def critic(name, mod, old, optim):
                return _ACPart(name, mod, old.module, optim, k[name], lambda t: Q.critic_flat_from_torch(t, o, a, dev, hidden=h),
                               lambda f: Q.critic_flat_to_torch(f, o, a, h, sizes=sz[name]), "adam_step", True)

            pol = self.policy
            return (_ACPart("pert", pol.actor_perturbation, self.actor_perturbation_target.module, self.actor_perturbation_optim,
                            k["pert"], lambda t: Q.pert_flat_from_torch(t, o, a, dev, hidden=h),
                            lambda f: Q.pert_flat_to_torch(f, o, a, h, d, sz["pert"]), "adam_step", True),
                    critic("critic1", pol.critic, self.critic_target, self.critic_optim),
                    critic("critic2", self.critic2, self.critic2_target, self.critic2_optim),
                    _ACPart("vae", pol.vae, None, self.vae_optim, k["vae"],
                            lambda t: Q.vae_flat_from_torch(t[:ne], t[ne:], o, a, ld, dev, hidden=hv), vae_to, "adam_step", True))

        def _engine(self):
            if self._hip_engine is None:
                flats = {p.name: p.flat() for p in self._hip_parts()}
                eng = Q.CBCQEngine(self._hip_obs_dim, self._hip_act_dim, self._hip_latent, flats["pert"], flats["critic1"],
                                   flats["critic2"], flats["vae"], Q.CBCQConfig(**self._hip_cbcq_fields()), hidden=self._hip_hidden,
                                   depth=self._hip_depth, activation=self._hip_actfn, vae_hidden=self._hip_vhidden,
                                   vae_depth=self._hip_vdepth, vae_activation=self._hip_vactfn)
                self._hip_engine = _ac_load(self, eng)         # resume: lagged networks, Adam moments / steps of a loaded checkpoint
            return self._hip_engine

        def _preprocess_batch(self, batch, buffer, indices):
            _ac_begin(self, who, buffer, indices)              # the mirror and the indices; the rows are gathered on the device
            return batch

        def _hip_noises(self, b: int, r: int, ld: int):
            """The three normal draws of one update, raw, in the reference's order: randn_like(std), decode(obs_next_rep)'s randn,
            decode(obs)'s randn."""
            if self._hip_update_noise == "torch":
                return torch.randn(b, ld), torch.randn(b * r, ld), torch.randn(b, ld)
            from .buffer import normal_noise

            key, c = self._hip_noise_key ^ 0xBC9, self._hip_noise_calls
            self._hip_noise_calls += 3
            return tuple(normal_noise(s, key, c + i, self._hip_device) for i, s in enumerate(((b, ld), (b * r, ld), (b, ld)), 1))

        def _hip_refresh_fields(self, eng) -> None:
            for k, v in self._hip_cbcq_fields().items():       # read at every update, as the learning rates
                if k == "num_sampled_action" and getattr(eng.cfg, k) != v:
                    raise NotImplementedError(f"{who}: `{k}` changed after the engine was built (call hip_invalidate())")
                setattr(eng.cfg, k, v)
            if int(self.policy.vae.latent_dim) != eng.latent_dim:
                raise NotImplementedError(f"{who}: `latent_dim` changed after the engine was built (call hip_invalidate())")

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            from .buffer import gather_rows_multi

            eng, m, idx = self._hip_engine, self._hip_mirror, self._hip_idx
            self._hip_refresh_fields(eng)
            obs, act, obs_next = gather_rows_multi([m.obs, m.act, m.obs_next], idx)
            rew, done = m.rew[idx].to(torch.float32), m.done[idx].to(torch.float32)
            stats = eng.update_with_batch(obs, act, rew, done, obs_next,
                                          *self._hip_noises(int(idx.numel()), eng.cfg.num_sampled_action, eng.latent_dim))
            s = stats.cpu().numpy()                                               # one D2H per update()
            self._hip_after_update()
            return BCQTrainingStats(actor_loss=float(s[0]), critic1_loss=float(s[1]), critic2_loss=float(s[2]), vae_loss=float(s[3]))

        def hip_policy_forward(self, obs, noise=None):
            """BCQPolicy.forward's actions for all observations in one engine call -> float32[N, act_dim] on the device.  `noise`:
            the raw normal draws [N, forward_sampled_times, latent_dim] (default: torch.randn, the reference's generator)."""
            _require_gpu(self._hip_device, who)
            eng = self._engine()
            self._hip_refresh_fields(eng)
            obs = torch.as_tensor(np.asarray(obs, np.float32) if not torch.is_tensor(obs) else obs)
            if noise is None:
                noise = torch.randn(obs.shape[0], eng.cfg.forward_sampled_times, eng.latent_dim)
            return eng.policy_forward(obs, noise)

        _hip_write_back = _ac_write_back

    return HipBCQ


# ---------------------------------------------------------------------------------------------------
# Branching DQN (bdqn.py:106-224) on BranchingNet: examples/box2d/bipedal_bdq.py
# ---------------------------------------------------------------------------------------------------
def make_hip_bdqn(ref=None):
    """Returns HipBDQN(BDQN): `_preprocess_batch` / `_update_with_batch` (bdqn.py:155-224) on the engine (tianshou_amd/bdqn.py).
    Supported model: BranchingNet with 1 .. 7 common hidden layers, at most one hidden layer in `value_hidden_sizes` and in
    `action_hidden_sizes`, widths up to 1024, ReLU or tanh, no norm_layer, num_branches <= 32, action_per_branch <= 64; Adam or
    RMSprop.  Anything else raises NotImplementedError naming this envelope (`bdqn.describe_model`); there is no torch fallback.
    `_preprocess_batch` takes obs_next / rew of the sampled batch and the buffer's end flags as the reference does and makes ONE
    target call; `batch.returns` is the device [B] result expanded as a view to [B, D, A].  `_update_with_batch` synchronises the
    lagged network first, then one update call; the signed sum_d td goes to `batch.weight`.  Unlike the reference at B = 1 with
    D > 1 (whose `.squeeze()` drops the batch axis) the target is the same formula at every B.  Like the reference, the targets
    discount with the default of `_compute_return`'s `gamma` argument (0.99), not with `BDQN(gamma=...)`.  The collector's
    `policy.forward` / `add_exploration_noise` stay the reference's.  `ref`: optional namespace replacing the tianshou imports
    (see `_ref`)."""
    from . import bdqn as BD

    SimpleLossTrainingStats = _ref(ref, "tianshou.algorithm.modelfree.reinforce", "SimpleLossTrainingStats")
    Base = _ref(ref, "tianshou.algorithm.modelfree.bdqn", "BDQN")

    class HipBDQN(_HipGlue, Base):
        def __init__(self, *args, device="cuda", **kwargs):
            super().__init__(*args, **kwargs)
            self._hip_device = torch.device(device)
            self._hip_desc = BD.describe_model(self.policy.model)            # raises NotImplementedError naming the envelope
            optimizer_fields(self.optim._optim)                             # (raises on an optimizer the engine does not implement)
            if float(self.gamma) != self._hip_target_gamma():
                import warnings

                warnings.warn(f"HipBDQN: gamma = {self.gamma} is not used by the targets: like the reference's BDQN they discount with "
                              f"the default of `_compute_return`'s `gamma` argument, {self._hip_target_gamma()}", stacklevel=2)
            self._hip_engine = None
            self._hip_glue_init()

        def _hip_qstate(self):
            return _QState(self._hip_desc["keys"], BD.flat_from_torch, BD.flat_to_torch, lambda eng: eng.dims)

        def _hip_config(self):
            of = optimizer_fields(self.optim._optim)
            return BD.BDQNConfig(gamma=self._hip_target_gamma(), target_update_freq=int(self.target_update_freq),
                                 is_double=bool(self.is_double), max_grad_norm=self.optim._max_grad_norm, **of)

        def _hip_target_gamma(self) -> float:
            """The discount of the targets.  bdqn.py:197-204 calls `_compute_return(batch, buffer, indices)` without its `gamma`
            argument, so the reference discounts with that signature's default (0.99) whatever `BDQN(gamma=...)` was given; the
            drop-in computes what the reference computes and reads the same default."""
            import inspect

            return float(inspect.signature(Base._compute_return).parameters["gamma"].default)

        def _engine(self):
            if self._hip_engine is None:
                dims = self._hip_desc["dims"]
                self._hip_engine = _q_load(self, BD.BDQNEngine(*dims, _q_flat(self, dims), self._hip_config()))
            return self._hip_engine

        def _hip_refresh_lr(self) -> None:
            super()._hip_refresh_lr()
            eng = self._hip_engine
            if eng is not None:                  # plain attributes of the algorithm, read at every update like the learning rate
                eng.cfg.gamma, eng.cfg.is_double = self._hip_target_gamma(), bool(self.is_double)
                eng.cfg.max_grad_norm = self.optim._max_grad_norm

        def _preprocess_batch(self, batch, buffer, indices):
            """bdqn.py:173-204: the 1-step target of the sampled transitions."""
            _require_gpu(self._hip_device, "HipBDQN")
            eng = self._engine()
            self._hip_refresh_lr()
            end = np.asarray(buffer.done).copy()                            # bdqn.py:184-186
            end[buffer.unfinished_index()] = True
            obs_next = batch.obs_next.obs if hasattr(batch.obs_next, "obs") else batch.obs_next
            ret = eng.target_q(np.asarray(obs_next, np.float32), np.asarray(batch.rew, np.float32), end[np.asarray(indices)])
            batch.returns = ret.view(-1, 1, 1).expand(-1, eng.D, eng.A)
            if hasattr(batch, "weight"):                                    # prio buffer (bdqn.py:193-194)
                batch.weight = torch.as_tensor(np.asarray(batch.weight), dtype=torch.float32, device=self._hip_device)
            return batch

        def _update_with_batch(self, batch):
            self._hip_refresh_lr()
            eng = self._engine()
            weight = batch.pop("weight", None)
            obs = batch.obs.obs if hasattr(batch.obs, "obs") else batch.obs
            ret = batch.returns[:, 0, 0]
            loss, prio = eng.update(np.asarray(obs, np.float32), np.asarray(batch.act, np.int64), ret, weight)
            self._iter = eng.iter
            batch.weight = prio                                             # prio-buffer, bdqn.py:221: signed
            self._hip_after_update()
            return SimpleLossTrainingStats(loss=float(loss.item()))

        _hip_write_back = _q_write_back

    return HipBDQN
