"""Which optimiser step an engine launches: `torch.optim.Adam` on trl_clip_adam_f32, `torch.optim.RMSprop` and
`torch.optim.SGD` on trl_clip_step_f32 (csrc/k_optim.hip).  The optimiser objects stay what the reference keeps them for
-- `param_groups` (the schedules write the learning rate there) and `state_dict` -- and their state is bound, under
torch's own names for the class, to slices of the engine's flat state buffers.

One difference from torch: an SGD with momentum has its (zero) `momentum_buffer` bound from the start, where torch's state
has none until the first step, and "first step" is the engine's device-resident step count being zero, not the buffer being
absent.  A checkpoint's non-zero `momentum_buffer` loaded into an engine that has not stepped yet is therefore overwritten
by the first-step rule `buf = g`; set the engine's `step_state` along with it."""
import torch
import torch.optim as optim

from .. import _C


def step_spec(optimizer):
    """("adam", eps) | ("rmsprop", alpha, eps, momentum, centered, weight_decay) | ("sgd", momentum, dampening, nesterov,
    weight_decay) of `optimizer`, read from its class and its first parameter group.  Hashable: the step-relevant
    hyper-parameters join the engines' graph-cache keys.  Any other class, and the options that change what a step
    computes or how torch would run it (`maximize`, `differentiable`, a `foreach` / `capturable` the user set), raise."""
    cls, g = type(optimizer), optimizer.param_groups[0]
    if cls is optim.Adam:
        return ("adam", float(g.get("eps", 1e-8)))
    if cls is not optim.RMSprop and cls is not optim.SGD:
        raise _C.TrlError("the HIP path steps torch.optim.Adam, torch.optim.RMSprop and torch.optim.SGD, not %s"
                          % getattr(cls, "__name__", cls))
    for flag in ("maximize", "differentiable", "capturable", "fused"):
        if g.get(flag):
            raise _C.TrlError("%s(%s=%r) has no kernel on the HIP path" % (cls.__name__, flag, g[flag]))
    if g.get("foreach") is not None:
        raise _C.TrlError("%s(foreach=%r): the HIP step is single-tensor torch.optim arithmetic; leave `foreach` unset"
                          % (cls.__name__, g["foreach"]))
    if cls is optim.RMSprop:
        return ("rmsprop", float(g["alpha"]), float(g["eps"]), float(g["momentum"]), bool(g["centered"]),
                float(g["weight_decay"]))
    return ("sgd", float(g["momentum"]), float(g["dampening"]), bool(g["nesterov"]), float(g["weight_decay"]))


def state_names(spec):
    """torch's state keys of the class, in the order of the flat state buffers (trl_opt_t's state0..2; Adam's m, v); None
    where the options keep no such buffer."""
    if spec[0] == "adam":
        return ("exp_avg", "exp_avg_sq")
    if spec[0] == "rmsprop":
        return ("square_avg", "momentum_buffer" if spec[3] > 0 else None, "grad_avg" if spec[4] else None)
    return ("momentum_buffer" if spec[1] != 0 else None,)


def needs_third(specs):
    """Only centered RMSprop keeps a third state buffer."""
    return any(s[0] == "rmsprop" and s[4] for s in specs)


def bind_state(optimizer, spec, plist, offset, buffers):
    """`optimizer.state[p]` of every parameter of `plist` (laid out from `offset` in the flat buffers) bound to its slices of
    `buffers` under `state_names(spec)`; returns the host `step` tensors it planted (SGD keeps none)."""
    steps, names = [], state_names(spec)
    for p in plist:
        n = p.numel()
        state = {}
        if spec[0] != "sgd":
            state["step"] = torch.tensor(0.0)
            steps.append(state["step"])
        for name, buf in zip(names, buffers):
            if name is not None:
                state[name] = buf[offset:offset + n].view(p.shape)
        optimizer.state[p] = state
        offset += n
    return steps


def step_args(spec, flat, grads, buffers, sizes, lrs, *, eps=None, **kw):
    """The descriptor of one clip + step launch for `spec`: `_C.AdamArgs` or `_C.OptArgs`.  `buffers` = (m, v, third or
    None); `eps`: Adam's, where the engine keeps its own."""
    if spec[0] == "adam":
        return _C.adam_args(flat, grads, buffers[0], buffers[1], sizes, lrs, eps=spec[1] if eps is None else eps, **kw)
    states = [buf if name is not None else None for name, buf in zip(state_names(spec), buffers)]
    return _C.opt_args(spec, flat, grads, states, sizes, lrs, **kw)


def clip_step(args, device):
    (_C.clip_adam if isinstance(args, _C.AdamArgs) else _C.clip_step)(args, device)


def clip_step_polyak(args, target, source, tau, device):
    (_C.clip_adam_polyak if isinstance(args, _C.AdamArgs) else _C.clip_step_polyak)(args, target, source, tau, device)
