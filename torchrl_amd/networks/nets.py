"""Net / QNet heads (torchrl/networks/nets.py:13-68) + the flat-parameter view
the HIP kernels consume.

A `Net` whose trunk is an `MLPBase` with two equal hidden widths, Tanh or ReLU,
no LayerNorm and no extra hidden layers is an "MLP2" block (include/trl_hip.h):
`mlp2_spec()` describes it and `flatten_mlp2()` re-homes its parameters as
views into ONE contiguous fp32 buffer  W1 b1 W2 b2 W3 b3 [logstd]  so kernels
read/write the very storage `state_dict()` / `parameters()` expose.

`forward` on a GPU MLP2 under no_grad runs trl_mlp2_forward_f32; other MLPs run
layer by layer on the dense-layer kernels, `add_ln=True` ones with their
LayerNorm layers on k_layernorm.hip in between (ops.net_plan).  With autograd
enabled (algorithms outside this repo's hot-path scope) it is the plain
nn.Module graph.

`BootstrappedNet` / `FlattenBootstrappedNet` (nets.py:71-127): K heads on one MLP trunk for Bootstrapped DQN; on the
GPU the trunk runs once and the requested heads as grouped launches into one head-major stack.
"""
import torch
import torch.nn as nn

from . import init
from .base import MLPBase
from .. import _C

_ACT_CODE = {nn.Tanh: _C.ACT_TANH, nn.ReLU: _C.ACT_RELU}


# Parameters that a launch sequence on ANOTHER stream is still stepping (the critic's half of a PPO epoch runs beside the
# next rollout, algo/on_policy/ppo.py): net -> the event that sequence ends with.  Whoever is about to read such a net's
# parameters on the current stream waits for the event first (`settle`); weak keys: nothing is kept alive, nothing is
# pickled or deep-copied with the module.
import weakref
_PENDING = weakref.WeakKeyDictionary()


def set_pending(net, event):
    if event is None:
        _PENDING.pop(net, None)
    else:
        _PENDING[net] = event


def pending_event(net):
    return _PENDING.get(net)


def settle(net, device=None):
    """Make the current stream wait for whatever is still writing `net`'s parameters on another stream.  Inside a stream
    capture this does nothing: the event was recorded outside the capture, and every capture site waits on the current
    stream before it captures or replays (`_FusedPPO._run_chains` / `run`, `VecOnPolicyCollector._rollout_per_step`)."""
    if isinstance(net, ZeroNet):                                     # no parameters: nothing can be stepping them
        return
    ev = _PENDING.get(net)
    if ev is not None and not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream(device).wait_event(ev)


class Net(nn.Module):
    def __init__(self, output_shape, base_type, append_hidden_shapes=[],
                 append_hidden_init_func=init.basic_init, net_last_init_func=init.uniform_init,
                 activation_func=nn.ReLU, add_ln=False, **kwargs):
        super().__init__()
        self.base = base_type(activation_func=activation_func, add_ln=add_ln, **kwargs)
        self.add_ln = add_ln
        self.activation_func = activation_func
        width = self.base.output_shape
        layers = []
        for nxt in append_hidden_shapes:
            fc = nn.Linear(width, nxt)
            append_hidden_init_func(fc)
            layers += [fc, activation_func()]
            if add_ln:
                layers.append(nn.LayerNorm(nxt))
            width = nxt
        last = nn.Linear(width, output_shape)
        net_last_init_func(last)
        layers.append(last)
        self.append_fcs = layers
        self.seq_append_fcs = nn.Sequential(*layers)
        self.out_dim = output_shape
        self._flat = None

    # ---- MLP2 description / flat storage ----
    def mlp2_spec(self):
        """(D, H, O, act_code) if this net is an MLP2 block the kernels support, else None."""
        b = self.base
        if not isinstance(b, MLPBase) or self.add_ln or len(self.append_fcs) != 1:
            return None
        if len(b.hidden_shapes) != 2 or b.hidden_shapes[0] != b.hidden_shapes[1]:
            return None
        if b.activation_func not in _ACT_CODE or b.last_activation_func is not b.activation_func:
            return None
        return (b.input_dim, b.hidden_shapes[0], self.out_dim, _ACT_CODE[b.activation_func])

    def _mlp2_param_list(self):
        lin = [m for m in self.base.seq_fcs if isinstance(m, nn.Linear)] + [self.append_fcs[-1]]
        out = []
        for l in lin:
            out += [l.weight, l.bias]
        return out

    def flat_params(self):
        """Contiguous fp32 buffer aliasing this net's parameters (built on first use and
        re-built if `.to()` / `load_state_dict` moved the storage)."""
        plist = self._mlp2_param_list() + self._extra_flat_params()
        flat = self._flat
        ok = flat is not None and flat.device == plist[0].device
        if ok:
            off = 0
            for p in plist:
                if p.data_ptr() != flat.data_ptr() + 4 * off or not p.is_contiguous():
                    ok = False
                    break
                off += p.numel()
        if not ok:
            flat = flatten_into(plist)
            self._flat = flat
        return flat

    def _extra_flat_params(self):
        return []

    # (whoever saves or loads the parameters reads / writes them on the current stream: settle first, like `forward`)
    def _settle_params(self):
        if _PENDING and self in _PENDING:
            p = next(self.parameters(), None)
            settle(self, p.device if p is not None and p.is_cuda else None)

    def state_dict(self, *args, **kwargs):
        self._settle_params()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._settle_params()
        return super().load_state_dict(*args, **kwargs)

    def forward(self, x):
        spec = self.mlp2_spec()
        needs_graph = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if x.is_cuda and _PENDING:
            settle(self, x.device)
        if x.is_cuda and not needs_graph:
            lead = x.shape[:-1]
            if spec is not None and _C.lib().trl_mlp2_forward_supported(spec[0], spec[1], spec[2]):
                D, H, O, act = spec                                 # fused 2-layer kernel
                x2 = x.reshape(-1, D).float().contiguous()
                return _C.mlp2_forward(self.flat_params(), x2, D, H, O, act).reshape(tuple(lead) + (O,))
            from .. import ops
            ln = self.add_ln and isinstance(self.base, MLPBase)
            try:
                # LayerNorm layers: k_layernorm.hip between the dense layers (ops.net_plan)
                layers, act = ops.net_layers(self) if ln else (ops.linear_layers(self), ops.act_code(self))
            except _C.TrlError:
                if ln and self.base.activation_func in ops.ACT_OF:
                    raise                                           # a norm the kernels do not carry: say so, do not go eager
                layers = None                                       # conv trunk / other activations: torch modules
            if layers is not None and isinstance(self.base, MLPBase):
                x2 = x.reshape(-1, int(layers[0][0].shape[1])).float().contiguous()
                if ops.has_post(layers):
                    out, _ = ops.mlp_forward(layers, x2, act, keep=False)
                else:
                    out, _ = ops.mlp_forward([(w.detach(), b.detach()) for w, b in layers], x2, act)   # dense-layer kernels
                return out.reshape(tuple(lead) + (self.out_dim,))
        if x.is_cuda:
            _C.note_eager(type(self).__name__ + ".forward", "autograd is on" if needs_graph else "no kernel for this trunk")
        return self.seq_append_fcs(self.base(x))


def flatten_into(plist):
    """Copy parameters into one buffer and turn them into views of it."""
    total = sum(p.numel() for p in plist)
    flat = torch.empty(total, dtype=torch.float32, device=plist[0].device)
    off = 0
    with torch.no_grad():
        for p in plist:
            n = p.numel()
            flat[off:off + n].copy_(p.detach().reshape(-1))
            p.data = flat[off:off + n].view(p.shape)
            off += n
    return flat


class FlattenNet(Net):
    def forward(self, input):
        return super().forward(torch.cat(input, dim=-1))


class QNet(Net):
    def forward(self, input):
        assert len(input) == 2, "Q Net only get observation and action"
        state, action = input
        return super().forward(torch.cat([state, action], dim=-1))


class BootstrappedNet(nn.Module):
    """K Q heads on one trunk (torchrl/networks/nets.py:71-121, Bootstrapped DQN).  Module names, construction order
    (trunk, then heads 0..K-1, hidden layers before the last layer inside a head) and initialisation are the
    reference's, so state dicts interchange and a seeded construction gives the same parameters: `base.*`, then
    `head{k}` = nn.Sequential([Linear, act] * len(append_hidden_shapes) + [Linear]).

    `forward(x, head_idxs)` returns the list of the requested heads' (..., A) outputs.  On the GPU under no_grad the trunk
    runs ONCE on the dense-layer kernels and all requested heads as one grouped launch per head level, written into one
    head-major (len(head_idxs), rows, A) stack (`forward_stack`) whose blocks are the returned tensors.

    Limits (each a loud _C.TrlError): MLP trunks only (a CNNBase trunk, the reference's Atari config, is not built), no
    LayerNorm (`add_ln=True`), 1 <= head_num <= 64 and 1 <= output_shape <= 64 (the sizes k_bootdqn.hip carries).

    TRL_BOOT_CONV=1 (`ops.boot_conv`, read in the constructor): `base_type=CNNBase | partial(CNNBase, ...)` constructs too
    (`is_conv`).  `trunk_layers()` / `param_list()` then give the conv W, b in `ops.cnn_param_list` order before the heads,
    `forward_stack` takes (rows, C, H, W) uint8 frame stacks -- the conv trunk once, up to the flattened feature, the heads
    as grouped launches -- and the eager `forward` stays what it is for CPU use.  Refused by name there as well: `add_ln`,
    padding / dilation / groups the conv kernels refuse, a trunk whose activation differs from the heads'."""

    def __init__(self, output_shape, base_type, head_num=10, append_hidden_shapes=[],
                 append_hidden_init_func=init.basic_init, net_last_init_func=init.uniform_init,
                 activation_func=nn.ReLU, add_ln=False, **kwargs):
        super().__init__()
        import functools
        from .base import CNNBase
        from .. import ops
        trunk_cls = base_type.func if isinstance(base_type, functools.partial) else base_type
        self.is_conv = isinstance(trunk_cls, type) and issubclass(trunk_cls, CNNBase) and ops.boot_conv()
        if not self.is_conv and not (isinstance(trunk_cls, type) and issubclass(trunk_cls, MLPBase)):
            raise _C.TrlError("BootstrappedNet over a %s trunk is not built: the Bootstrapped DQN path runs MLP trunks "
                              "(networks.MLPBase) only, conv trunks are outside it" % getattr(trunk_cls, "__name__", trunk_cls))
        if add_ln:
            raise _C.TrlError("BootstrappedNet(add_ln=True) is not built: the grouped head launches carry no LayerNorm")
        if not 1 <= int(head_num) <= 64:
            raise _C.TrlError("BootstrappedNet: the Bootstrapped DQN kernels carry 1..64 heads, got head_num=%s" % (head_num,))
        if not 1 <= int(output_shape) <= 64:
            raise _C.TrlError("BootstrappedNet: the Bootstrapped DQN kernels carry 1..64 actions, got output_shape=%s"
                              % (output_shape,))
        self.base = base_type(activation_func=activation_func, add_ln=add_ln, **kwargs)
        self.add_ln = add_ln
        self.activation_func = activation_func
        if self.is_conv:
            ops.conv_layers(self)                                        # (padding / dilation / groups the conv kernels refuse)
            if self.base.activation_func is not activation_func or self.base.last_activation_func is not activation_func:
                raise _C.TrlError("BootstrappedNet: the conv trunk's activation (%s, last %s) differs from the heads' (%s): "
                                  "trunk and heads run one activation"
                                  % (getattr(self.base.activation_func, "__name__", self.base.activation_func),
                                     getattr(self.base.last_activation_func, "__name__", self.base.last_activation_func),
                                     getattr(activation_func, "__name__", activation_func)))
        self.head_num = int(head_num)
        self.out_dim = int(output_shape)
        self.bootstrapped_heads = []
        for idx in range(self.head_num):
            width = self.base.output_shape
            layers = []
            for nxt in append_hidden_shapes:
                fc = nn.Linear(width, nxt)
                append_hidden_init_func(fc)
                layers += [fc, activation_func()]
                width = nxt
            last = nn.Linear(width, output_shape)
            net_last_init_func(last)
            layers.append(last)
            head = nn.Sequential(*layers)
            setattr(self, "head{}".format(idx), head)
            self.bootstrapped_heads.append(head)

    def trunk_layers(self):
        """(W, b) per trunk layer: the Linear layers of an MLP trunk, the Conv2d layers (W 4-D, `ops.cnn_param_list`'s
        order) of a conv trunk."""
        if self.is_conv:
            return [(m.weight, m.bias) for m in self.base.seq_convs if isinstance(m, nn.Conv2d)]
        return [(m.weight, m.bias) for m in self.base.seq_fcs if isinstance(m, nn.Linear)]

    def head_layers(self, idx):
        return [(m.weight, m.bias) for m in self.bootstrapped_heads[idx] if isinstance(m, nn.Linear)]

    def param_list(self):
        """Trunk, then heads 0..K-1: W, b per layer -- the order of the engine's flat buffer (and of `parameters()`)."""
        out = []
        for w, b in self.trunk_layers() + [wb for k in range(self.head_num) for wb in self.head_layers(k)]:
            out += [w, b]
        return out

    def forward_stack(self, x, head_idxs=None):
        """The heads' Q values as one head-major (len(head_idxs), rows, A) stack, on the kernels (no autograd):
        one trunk pass, one grouped launch per head level."""
        from .. import ops
        idxs = list(range(self.head_num)) if head_idxs is None else [int(i) for i in head_idxs]
        if not idxs or any(not 0 <= i < self.head_num for i in idxs):
            raise _C.TrlError("BootstrappedNet: head indices must lie in [0, %d), got %s" % (self.head_num, idxs))
        if self.is_conv:
            # (rows, C, H, W) uint8 frame stacks: the conv trunk once, up to the flattened feature
            act = ops.cnn_act_code(self)
            feat, _ = ops.cnn_forward(self, x.reshape((-1,) + tuple(x.shape[-3:])), feature=True)
        else:
            act = ops.act_code(self)
            trunk = [(w.detach(), b.detach()) for w, b in self.trunk_layers()]
            x2 = x.reshape(-1, int(trunk[0][0].shape[1])).float().contiguous()
            feat, _ = ops.mlp_forward(trunk, x2, act, last_act=act, keep=False)
        stack = torch.empty((len(idxs), int(feat.shape[0]), self.out_dim), dtype=torch.float32, device=x.device)
        heads = [[(w.detach(), b.detach()) for w, b in self.head_layers(i)] for i in idxs]
        ops.mlp_forward_group(heads, [feat] * len(idxs), act, keep=[False] * len(idxs), out=list(stack.unbind(0)))
        return stack

    def forward(self, x, head_idxs):
        needs_graph = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if x.is_cuda and not needs_graph:
            lead = tuple(x.shape[:-3]) if self.is_conv else tuple(x.shape[:-1])
            return [q.reshape(lead + (self.out_dim,)) for q in self.forward_stack(x, head_idxs).unbind(0)]
        if x.is_cuda:
            _C.note_eager(type(self).__name__ + ".forward", "autograd is on")
        feature = self.base(x)
        return [self.bootstrapped_heads[idx](feature) for idx in head_idxs]


class FlattenBootstrappedNet(BootstrappedNet):
    def forward(self, input, head_idxs):
        return super().forward(torch.cat(input, dim=-1), head_idxs)


class ZeroNet(nn.Module):
    """The vacant critic of REINFORCE (torchrl/networks/nets.py, reinforce.py:20-21): V == 0.  The collector, the epoch
    post-processing and `settle` recognise it by type and never call it."""

    def forward(self, x):
        return torch.zeros(1)
