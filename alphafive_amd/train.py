"""Training step of the reference (genData/network.py:40-50 loss graph, main.py:38-39,62-75 loop) on
PyTorch-ROCm, so self-play -> replay -> update closes on one node without TensorFlow.  SURVEY §8f
rank 2: a caller of the hot path, not part of it.

    total = -mean(w * sum(pi * log_softmax(z)))  +  2 * mean(w * (v - z_v)^2)  +  4e-5 * sum_k ||k||^2 / 2
            (kernels only: variables whose name contains "bias" are excluded, network.py:48)
    optimiser: tf.train.AdamOptimizer(lr) semantics (beta1 .9, beta2 .999, eps 1e-8 added to sqrt(v) AFTER
               folding the bias corrections into the step size), lr from config.get_lr(step) (config.py:9,23-27)
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import tensorbundle
from .network import _BLOCKS, variable_shapes


def forward_train(params, x):
    """Differentiable forward on TF-layout parameters -> (logits[B,S*S], value[B])."""
    def conv(h, name, act):
        k = params[name + "/kernel"].permute(3, 2, 0, 1)
        y = F.conv2d(h, k, params[name + "/bias"], padding=k.shape[-1] // 2)
        return F.elu(y) if act else y

    def residual(h, name):
        return F.elu(conv(h, name + "_res", False) + conv(conv(h, name + "_conv1", True), name + "_conv2", False))

    B = x.shape[0]
    f = conv(x, "bone/conv1", True)
    f = residual(f, "bone/block1")
    f = residual(f, "bone/block2")
    v = residual(f, "value/block3")
    v = conv(v, "value/conv", True).reshape(B, -1)
    v = F.elu(v @ params["value/fc1/kernel"] + params["value/fc1/bias"])
    v = torch.tanh((v @ params["value/fc2/kernel"] + params["value/fc2/bias"]) / 2).squeeze(1)
    p = residual(f, "policy/block4")
    p = residual(p, "policy/block5")
    p = conv(p, "policy/conv", True).reshape(B, -1)
    return p @ params["policy/fc/kernel"] + params["policy/fc/bias"], v


def forward_train_deep(params, x):
    """Differentiable forward of network_deep.DeepResNet on its named parameters (network_deep.variable_shapes: OIHW kernels,
    [in][out] dense layers; the block count is read off the names) -> (logits[B,S*S], value[B]).  The torch ops of
    DeepResNet.eval_device in the same order, so on fp32 parameters it gives eval_device(dtype=float32)'s bits."""
    def wb(name):
        return params[name + "/kernel"], params[name + "/bias"]

    B = x.shape[0]
    h = F.elu(F.conv2d(x, *wb("stem"), padding=2))
    b = 0
    while "tower/block%d_res/kernel" % b in params:
        r = F.conv2d(h, *wb("tower/block%d_res" % b))
        g = F.elu(F.conv2d(h, *wb("tower/block%d_conv1" % b), padding=1))
        h = F.elu(r + F.conv2d(g, *wb("tower/block%d_conv2" % b), padding=1))
        b += 1
    v = F.elu(F.conv2d(h, *wb("value/conv"))).reshape(B, -1)
    v = F.elu(v @ params["value/fc1/kernel"] + params["value/fc1/bias"])
    v = torch.tanh((v @ params["value/fc2/kernel"] + params["value/fc2/bias"]).float() / 2).squeeze(1)
    p = F.elu(F.conv2d(h, *wb("policy/conv"))).reshape(B, -1)
    return (p @ params["policy/fc/kernel"] + params["policy/fc/bias"]).float(), v


def loss_terms(params, boards, distrib, winner, weights, forward=forward_train):
    """network.py:40-50 -> dict(total, cross_entropy, value_loss, entropy).  `forward`: (params, boards) -> (logits, value),
    the 42-variable net's by default, forward_train_deep for network_deep.DeepResNet."""
    logits, value = forward(params, boards)
    logsm = F.log_softmax(logits, dim=1)
    x_entropy = (distrib * logsm).sum(dim=1)
    value_sq = (value - winner) ** 2
    l2 = sum((p ** 2).sum() / 2 for n, p in params.items() if "bias" not in n and "bn" not in n)
    total = -(x_entropy * weights).mean() + 2.0 * (value_sq * weights).mean() + 4e-5 * l2
    entropy = -(F.softmax(logits, dim=1) * logsm).sum(dim=1).mean()
    return dict(total=total, cross_entropy=-x_entropy.mean(), value_loss=value_sq.mean(), entropy=entropy)


class Trainer(object):
    """Holds the variables as torch parameters (TF layout/names) + TF-style Adam slots.  The update of the 42 variables is nine
    multi-tensor launches instead of ~210 per-variable ones (at the reference's batch of 512 the step is launch-bound:
    7.4 -> 6.0 ms, tools/probe_train_step.py); step(..., metrics=False) returns None and never waits for the device.

    fused=True (a CUDA/ROCm device only) takes everything but the network itself out of PyTorch: the loss head with its gradient,
    Adam with the L2 gradient and the L2 sum, and the logged scalars are three HIP launches (train_hip, include/af_train.h)
    around one torch.autograd.grad through the convolutions and dense layers.  `total`'s graph — the 21 per-variable L2 sums
    among it — is never built.  The variables, `m` and `v` then live in one flat buffer each; params / m / v are views into
    them under the same names and shapes, so everything below reads and writes them as before."""

    def __init__(self, variables, board_size, device=None, beta1=0.9, beta2=0.999, eps=1e-8, forward=None, shapes=None,
                 fused=False):
        """`forward` / `shapes`: the differentiable forward and the {name: shape} table of the net to train; by default the
        42-variable net's (forward_train, network.variable_shapes).  DeepResNet: forward_train_deep, net.variable_shapes()."""
        self.board_size = board_size
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.forward = forward if forward is not None else forward_train
        self.fused = bool(fused)
        if self.fused and self.device.type != "cuda":
            raise ValueError("Trainer(fused=True) runs HIP kernels (libaf_train.so) and needs a CUDA/ROCm device, not %r: "
                             "there is no host version of them to fall back to" % str(self.device))
        shapes = shapes if shapes is not None else variable_shapes(board_size)
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self.t = 0
        if self.fused:
            self._init_fused(variables, shapes)
            return
        self.params = {k: torch.tensor(np.asarray(variables[k], np.float32), device=self.device, requires_grad=True)
                       for k in shapes}
        self.m = {k: torch.zeros_like(p) for k, p in self.params.items()}
        self.v = {k: torch.zeros_like(p) for k, p in self.params.items()}
        self._lr_t = torch.zeros((), dtype=torch.float32, device=self.device)

    def _init_fused(self, variables, shapes):
        """One flat buffer each for the variables, m and v; params / m / v are views into them (the parameters leaves that
        require grad: a view of a tensor that does not is a leaf).  The Adam table is built once: these pointers never move."""
        from . import train_hip
        train_hip.lib()                                     # a missing library is an error here, not at the first step
        sizes = {k: int(np.prod(shp, dtype=np.int64)) for k, shp in shapes.items()}
        total = sum(sizes.values())
        host = np.empty(total, np.float32)
        views, off = {}, 0
        for k, shp in shapes.items():
            a = np.asarray(variables[k], np.float32)
            if tuple(a.shape) != tuple(shp):
                raise ValueError("variable %s has shape %s, expected %s" % (k, a.shape, tuple(shp)))
            host[off:off + sizes[k]] = a.reshape(-1)
            views[k] = (off, off + sizes[k], tuple(shp))
            off += sizes[k]
        self._flat = dict(params=torch.from_numpy(host).to(self.device),
                          m=torch.zeros(total, dtype=torch.float32, device=self.device),
                          v=torch.zeros(total, dtype=torch.float32, device=self.device))
        cut = lambda flat: {k: flat[a:b].view(shp) for k, (a, b, shp) in views.items()}
        self.params = {k: p.requires_grad_(True) for k, p in cut(self._flat["params"]).items()}
        self.m, self.v = cut(self._flat["m"]), cut(self._flat["v"])
        names = list(shapes)
        self._table = train_hip.VarTable([self.params[k] for k in names], [self.m[k] for k in names],
                                         [self.v[k] for k in names], ["bias" not in k and "bn" not in k for k in names])
        self._l2_partials = torch.zeros(max(1, self._table.n_partials), dtype=torch.float32, device=self.device)
        self._lr_t = 0.0                                    # a kernel argument on this path, not a device scalar

    def _update_fused(self, batch):
        """forward -> loss head (d total / d logits, d total / d value without the L2 term) -> autograd through the network ->
        Adam (adds the L2 gradient l2_coef * p itself, sums p^2 on the way) -> the four scalars, all on the device."""
        from . import train_hip
        boards, distrib, winner, weights = batch
        ps = list(self.params.values())
        logits, value = self.forward(self.params, boards)
        dlogits, dvalue, rows = train_hip.loss_head(logits, value, distrib.contiguous(), winner.contiguous(),
                                                    weights.contiguous())
        self._table.set_grads(torch.autograd.grad([logits, value], ps, [dlogits, dvalue]))
        n = train_hip.adam(self._table, self._lr_t, self.beta1, self.beta2, self.eps, train_hip.L2_COEF, self._l2_partials)
        terms = train_hip.finalize(rows, self._l2_partials, n, train_hip.L2_COEF)
        return dict(total=terms[0], cross_entropy=terms[1], value_loss=terms[2], entropy=terms[3])

    def _update(self, batch):
        """loss -> gradients -> Adam (tf.train.AdamOptimizer: lr_t folds the bias corrections, eps is added to sqrt(v)).
        Same arithmetic order as the per-variable loop it replaces: p -= (lr_t * m) / (sqrt(v) + eps)."""
        if self.fused:
            return self._update_fused(batch)
        terms = loss_terms(self.params, *batch, forward=self.forward)
        ps = list(self.params.values())
        grads = list(torch.autograd.grad(terms["total"], ps))
        ms, vs = list(self.m.values()), list(self.v.values())
        with torch.no_grad():
            torch._foreach_mul_(ms, self.beta1)
            torch._foreach_add_(ms, grads, alpha=1.0 - self.beta1)
            torch._foreach_mul_(vs, self.beta2)
            torch._foreach_addcmul_(vs, grads, grads, value=1.0 - self.beta2)
            den = torch._foreach_sqrt(vs)
            torch._foreach_add_(den, self.eps)
            num = torch._foreach_mul(ms, self._lr_t)
            torch._foreach_div_(num, den)
            torch._foreach_sub_(ps, num)
        return {k: v.detach() for k, v in terms.items()}

    def step(self, boards, weights, values, policies, lr, metrics=True):
        """One optimiser step on a RandomStack.get_data batch (main.py:63-68). Returns the scalar metrics."""
        def to(a):      # numpy batches (utils.RandomStack) or device tensors (replay.DeviceRandomStack)
            if torch.is_tensor(a):
                return a.to(device=self.device, dtype=torch.float32)
            return torch.as_tensor(np.asarray(a, np.float32), device=self.device)
        batch = (to(boards), to(policies), to(values), to(weights))
        self.t += 1
        lr_t = float(lr * np.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t))
        if self.fused:
            self._lr_t = lr_t
        else:
            self._lr_t.fill_(lr_t)
        terms = self._update(batch)
        return {k: float(v) for k, v in terms.items()} if metrics else None

    def variables(self):
        return {k: p.detach().cpu().numpy().copy() for k, p in self.params.items()}

    def device_variables(self):
        """{name: parameter tensor, detached} on the trainer's device: no copy — the tensors the next step() writes into
        (ResNet.set_variables_device takes its own snapshot)."""
        return {k: p.detach() for k, p in self.params.items()}

    def save(self, ckpt_dir, step):
        """main.py:73-74 — a checkpoint the reference's ResNet.restore() can load."""
        os.makedirs(ckpt_dir, exist_ok=True)
        name = "alphaFive-%d" % step
        tensorbundle.save_bundle(os.path.join(ckpt_dir, name), self.variables())
        tensorbundle.write_checkpoint_state(ckpt_dir, name)

    # ---- optimiser state: what a run needs beyond the bundle to continue as if it had not stopped ----
    def state_dict(self):
        """-> dict(params, m, v: {name: float32 array}, t: int), host copies."""
        host = lambda d: {k: x.detach().cpu().numpy().copy() for k, x in d.items()}
        return dict(params=host(self.params), m=host(self.m), v=host(self.v), t=int(self.t))

    def load_state_dict(self, state):
        """Put a state_dict() back (in place: the parameter tensors keep their identity).  `m`, `v` and `t` may be missing —
        a bundle alone — and then stay as they are."""
        with torch.no_grad():
            for key, dst in (("params", self.params), ("m", self.m), ("v", self.v)):
                src = state.get(key)
                if src is None:
                    continue
                for k, x in dst.items():
                    a = np.asarray(src[k], np.float32)
                    if tuple(a.shape) != tuple(x.shape):
                        raise ValueError("%s[%s] has shape %s, expected %s" % (key, k, a.shape, tuple(x.shape)))
                    x.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        if state.get("t") is not None:
            self.t = int(state["t"])

    @staticmethod
    def _sidecar(ckpt_dir, step):
        return os.path.join(ckpt_dir, "alphaFive-%d.opt.npz" % step)

    def save_state(self, ckpt_dir, step):
        """Adam's slots and step count as a sidecar alphaFive-<step>.opt.npz beside the bundle save() wrote.  The bundle itself
        stays what the reference's ResNet.restore expects: variables only (the reference's own checkpoints hold no slots
        either: its Saver is created before its optimiser)."""
        os.makedirs(ckpt_dir, exist_ok=True)
        st = self.state_dict()
        arrays = {"m/" + k: a for k, a in st["m"].items()}
        arrays.update({"v/" + k: a for k, a in st["v"].items()})
        np.savez(self._sidecar(ckpt_dir, step), t=np.int64(st["t"]), **arrays)

    def load_state(self, ckpt_dir, step):
        """The variables of bundle alphaFive-<step> and the slots of its sidecar."""
        variables = tensorbundle.load_bundle(os.path.join(ckpt_dir, "alphaFive-%d" % step))
        with np.load(self._sidecar(ckpt_dir, step)) as z:
            m = {k[2:]: z[k] for k in z.files if k.startswith("m/")}
            v = {k[2:]: z[k] for k in z.files if k.startswith("v/")}
            t = int(z["t"])
        self.load_state_dict(dict(params=variables, m=m, v=v, t=t))


def _save_buffer(stack, step):
    if hasattr(stack, "save_pickles"):                  # replay.DeviceRandomStack: read out of HBM, same three files
        stack.save_pickles(step)
    else:
        os.makedirs("data_buffer", exist_ok=True)
        stack.save(step)                                # main.py:75


def train_loop(config, engine, net, stack, trainer, steps, log=print, start_step=1, resumable=False, ckpt_every=60,
               weights_on_device=False, device_draws=False):
    """main.py:57-76 with the five gen_data processes replaced by the device batch `engine`
    (alphafive_amd.engine.SelfPlayEngine): every accepted episode triggers 4 minibatches once the buffer is full.

    Every `ckpt_every` steps the weights are saved as a bundle the reference restores.  With resumable=True each of these is
    followed by the optimiser sidecar (Trainer.save_state) and the replay buffer (the reference's data_buffer/*.pkl under the
    current directory, main.py:75), so that resume() can hand back `start_step` for a run that continues this one.

    The self-play engine is not snapshotted.  Its trees are by far the largest state of the loop — at BASELINE configs[1] four
    edge arrays of 4096 games x 2064 nodes x 128 cells x 4 B, ~17 GB of HBM — and what a restart loses is only the games in
    flight: 4096 of them, ~17 s of self-play at ~240 episodes/s.  The caller's part: build the resumed run's engine with a
    `seed` / `first_game_id` the first run did not use, or it replays the same noise streams and plays the same games again.

    weights_on_device=True hands the new weights to the engine's evaluator without the host: net.set_variables_device(
    trainer.device_variables()) snapshots the parameters on the device and the evaluator re-packs them in place
    (af_net_update_device) instead of 42 device-to-host copies, a host re-pack and a reallocation of the evaluator per step.
    `net` may be a network_deep.DeepResNet with a Trainer built on forward_train_deep: its set_variables_device re-packs the
    bf16 tower in place (af_tower_update_device: launches only).

    device_draws=True takes the minibatch draws off the host too: the four minibatches of an accepted episode come from ONE
    stack.draw_batches(config.batch_size, 4) (replay.DeviceRandomStack: positions, turns and flips drawn by a counter-based
    generator on the device, keyed by the stack's draw_seed and draw_counter) and the four steps take its slices — four
    independent draws from the same buffer state, as the reference's four get_data calls are, but not from its global streams.
    A stack without draw_batches is a ValueError."""
    if device_draws and not hasattr(stack, "draw_batches"):
        raise ValueError("device_draws=True needs a stack with draw_batches (replay.DeviceRandomStack); %s has none" %
                         type(stack).__name__)
    step = start_step
    on_device = hasattr(stack, "iter_push_packed") and hasattr(engine, "post_episodes_device")
    cap = 256
    while step < steps:
        engine.run_ticks(256)
        engine.check()
        if on_device:       # episodes never leave the GPU: packed by the engine, decoded into the replay ring by one launch each
            pushes = stack.iter_push_packed(engine.post_episodes_device(cap), cap, config.gamma)
        else:
            pushes = (stack.push(data_record, result) for data_record, result in engine.pop_episodes())
        for r in pushes:                                # every finished episode reaches the buffer, also after the last step
            if r and stack.is_full() and step < steps:
                if device_draws:
                    drawn = stack.draw_batches(config.batch_size, 4)
                for i in range(4):                              # (only the last minibatch's scalars are logged: one sync per episode)
                    if device_draws:
                        boards, weights, values, policies = (t[i] for t in drawn)
                    else:
                        boards, weights, values, policies = stack.get_data(batch_size=config.batch_size)
                    metrics = trainer.step(boards, weights, values, policies, config.get_lr(step), metrics=i == 3)
                step += 1
                if weights_on_device:                           # the engine's evaluator follows the trainer
                    net.set_variables_device(trainer.device_variables())
                else:
                    net.set_variables(trainer.variables())
                log("step: %d, xcross_loss: %0.3f, mse: %0.3f, entropy: %0.3f" %
                    (step, metrics["cross_entropy"], metrics["value_loss"], metrics["entropy"]))
                if step % ckpt_every == 0:
                    trainer.save(config.ckpt_path, step)
                    if resumable:
                        trainer.save_state(config.ckpt_path, step)
                        _save_buffer(stack, step)
        if on_device:
            # a packed append that found its buffer not to hold what the header said appends nothing and raises a device flag,
            # while the host bookkeeping has already advanced: surface it here, once per hand-off, before the ring is sampled again
            stack.check()
    return step


def resume(config, net, stack, trainer, log=print):
    """Continue from the newest checkpoint the `checkpoint` file in config.ckpt_path names (main.py:29-34 restore=True): its
    variables go into `trainer` and `net`, the optimiser sidecar into `trainer` if there is one (if not, Adam starts fresh, as
    it does in the reference, whose checkpoints hold no slots), the buffer files of that step into `stack` if they exist.
    Returns the step to pass to train_loop as `start_step`.  The engine starts from empty boards: see train_loop.
    The stack's draw_counter (train_loop(device_draws=True)) is not restored either: build the continued run's stack with a
    `draw_seed` the first run did not use, or it draws the first run's minibatch selections again."""
    prefix = tensorbundle.resolve_checkpoint(config.ckpt_path)
    ckpt_dir, name = os.path.dirname(prefix), os.path.basename(prefix)
    step = int(name.rsplit("-", 1)[1])
    if os.path.exists(Trainer._sidecar(ckpt_dir, step)):
        trainer.load_state(ckpt_dir, step)
    else:
        trainer.load_state_dict(dict(params=tensorbundle.load_bundle(prefix)))
        log("no optimiser state beside %s: Adam starts fresh" % prefix)
    net.set_variables(trainer.variables())
    if all(os.path.exists("data_buffer/%s%d.pkl" % (stem, step)) for stem in ("data", "data_len", "result")):
        if hasattr(stack, "load_pickles"):
            stack.load_pickles(step)
        else:
            stack.load(step)
    else:
        log("no replay buffer saved at step %d: the buffer fills from self-play" % step)
    log("resumed from %s at step %d" % (prefix, step))
    return step
