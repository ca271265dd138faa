"""FusedAdam: torch.optim.Adam's interface and state (train.py:79 constructs
``optim.Adam(params, lr=1e-4, weight_decay=1e-4)``), one HIP pass over every
parameter per step (hkp_adam_step, csrc/adam.hip).

Same constructor, ``step()``, ``zero_grad()``, ``state_dict()`` / ``load_state_dict()``
and per-parameter state keys (``step``, ``exp_avg``, ``exp_avg_sq``) as
torch.optim.Adam, so checkpoints move between the two.  Options the reference
never uses (amsgrad, maximize, capturable, differentiable, fused, foreach,
decoupled weight decay) are rejected rather than silently ignored.  No CPU path:
parameters must be fp32 CUDA tensors.

Two options the reference does not have, both off by default (then ``step()`` is
the hkp_adam_step launches above and nothing else), both per param group:

``max_grad_norm``: clip the gradients by their global L2 norm, as
``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` before the step would.
The norm runs over the gradients of ALL groups of one ``step()`` (hkp_grad_norm:
fp64, fixed order, the same bits on every run); norm and coefficient stay on the
device (``opt.grad_norm``, ``opt.clip_coef``: 0-d tensors of the last step —
reading them is the caller's synchronisation), and the Adam pass of every group
that sets the option reads ``g * coef`` (hkp_adam_step_ex); ``p.grad`` keeps the
unscaled gradient.  Groups that set it must agree on the value.

``ema_decay`` (0.5 < d < 1): an exponential moving average of the group's
parameters in ``state[p]["ema"]``, a clone of ``p`` when first needed, then
``ema = ema + (1 - d) * (p - ema)`` after each update, in the same pass
(torch.optim.swa_utils' EMA, ``_foreach_lerp_``).  It travels in ``state_dict()``;
a loaded state without it (torch Adam's) re-creates it from the parameters.
``ema_parameters()`` lists it, ``with opt.ema_weights():`` runs a block on it.
"""
import contextlib
import ctypes
import math

import torch

from ._lib import AdamTensor, HkpError, call, lib

OPTION_KEYS = ("max_grad_norm", "ema_decay")


def _check_options(max_grad_norm, ema_decay):
    if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
        raise ValueError("FusedAdam: max_grad_norm must be > 0, got %r" % (max_grad_norm,))
    if ema_decay is not None and not 0.5 < float(ema_decay) < 1.0:
        raise ValueError("FusedAdam: ema_decay must lie strictly between 0.5 and 1, got %r" % (ema_decay,))


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                 max_grad_norm=None, ema_decay=None):
        if amsgrad or maximize or capturable or differentiable or fused:
            raise HkpError("FusedAdam: amsgrad/maximize/capturable/differentiable/fused are not supported")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("FusedAdam: invalid lr/eps/weight_decay")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedAdam: invalid betas %s" % (betas,))
        _check_options(max_grad_norm, ema_decay)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        max_grad_norm=max_grad_norm, ema_decay=ema_decay)
        super().__init__(params, defaults)
        # per param group: the launch table of the last step (parameter / moment
        # pointers fixed; gradient pointers refreshed each step) and the common step
        # count — rebuilding it per parameter in Python left the GPU idle ~1.4 ms per
        # training step.  Invalidated by load_state_dict / add_param_group.
        self._fast = {}
        # clipping: the gradient table over all groups (refreshed like the above), the
        # fp64 scratch and the [norm, coef] pair, allocated once
        self._norm = None
        self._norm_ws = None
        self._norm_out = None
        self.grad_norm = None
        self.clip_coef = None

    def load_state_dict(self, state_dict):
        self._fast = {}
        self._norm = None
        kept = [{k: g.get(k) for k in OPTION_KEYS} for g in self.param_groups]
        super().load_state_dict(state_dict)
        # a torch.optim.Adam state dict has neither option: this optimizer's stay
        for group, old in zip(self.param_groups, kept):
            for k in OPTION_KEYS:
                group.setdefault(k, old[k])
            _check_options(group["max_grad_norm"], group["ema_decay"])

    def add_param_group(self, param_group):
        self._fast = {}
        self._norm = None
        if isinstance(param_group, dict):
            _check_options(param_group.get("max_grad_norm"), param_group.get("ema_decay"))
        super().add_param_group(param_group)

    # ------------------------------------------------------------------ clipping

    def _max_grad_norm(self):
        vals = {float(g["max_grad_norm"]) for g in self.param_groups if g.get("max_grad_norm") is not None}
        if len(vals) > 1:
            raise HkpError("FusedAdam: param groups disagree on max_grad_norm (%s): one norm, one threshold"
                           % sorted(vals))
        return vals.pop() if vals else None

    def _norm_launch(self, arr, ps, max_norm):
        """hkp_grad_norm on a table whose gradient pointers are this step's: norm and
        coefficient stay on the device (self._norm_out, allocated once)."""
        dev = ps[0].device
        need = int(lib().hkp_grad_norm_partials(len(ps), arr))          # host only
        if self._norm_ws is None or self._norm_ws.numel() < need or self._norm_ws.device != dev:
            self._norm_ws = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
        if self._norm_out is None or self._norm_out.device != dev:
            self._norm_out = torch.zeros(2, dtype=torch.float32, device=dev)
            self.grad_norm, self.clip_coef = self._norm_out[0], self._norm_out[1]
        call("hkp_grad_norm", len(ps), arr, max_norm, ctypes.c_void_p(self._norm_ws.data_ptr()),
             self._norm_ws.numel(), ctypes.c_void_p(self._norm_out.data_ptr()),
             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    def _grad_norm(self, max_norm):
        """The norm over every group's gradients from a table of its own (cached like
        the step's; one group on its fast path shares the step's table instead)."""
        ps = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if not ps:
            return False
        nc = self._norm
        if nc is None or len(ps) != len(nc["ps"]) or any(a is not b for a, b in zip(ps, nc["ps"])):
            arr = (AdamTensor * len(ps))()
            for i, p in enumerate(ps):
                if p.dtype != torch.float32 or p.device.type != "cuda" or p.device != ps[0].device:
                    raise HkpError("FusedAdam: max_grad_norm needs fp32 CUDA parameters on one device")
                arr[i].n = p.numel()
            nc = self._norm = dict(ps=ps, arr=arr)
        arr = nc["arr"]
        for i, p in enumerate(ps):
            g = p.grad
            if g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous() or g.device != p.device:
                raise HkpError("FusedAdam: fp32 contiguous CUDA gradients only")
            arr[i].grad = g.data_ptr()
        self._norm_launch(arr, ps, max_norm)
        return True

    # ----------------------------------------------------------------------- EMA

    def _ema_of(self, p):
        st = self.state[p]
        if "ema" not in st:
            st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
        return st["ema"]

    def ema_parameters(self):
        """The EMA tensors of every group that sets ema_decay, in parameter order
        (created as clones of the parameters where they do not exist yet)."""
        return [self._ema_of(p) for group in self.param_groups if group.get("ema_decay") is not None
                for p in group["params"]]

    def _exchange_ema(self):
        ps = [p for group in self.param_groups if group.get("ema_decay") is not None for p in group["params"]]
        if not ps:
            raise HkpError("FusedAdam: ema_weights() without ema_decay")
        es = [self._ema_of(p) for p in ps]
        with torch.no_grad():
            # in-place copies: the pointers of the launch tables stay, the version
            # counters the packed-weight caches are keyed on move
            tmp = [p.detach().clone() for p in ps]
            torch._foreach_copy_(ps, es)
            torch._foreach_copy_(es, tmp)

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the block with parameters and EMA exchanged in place (evaluation,
        checkpoints); exchanged back on exit, also on an exception."""
        self._exchange_ema()
        try:
            yield self
        finally:
            self._exchange_ema()

    # ---------------------------------------------------------------------- step

    def _fast_table(self, gi, group):
        """The cached table of the group with this step's gradient pointers, or None
        (cache miss: slow path)."""
        fc = self._fast.get(gi)
        if fc is None:
            return None
        if (group.get("ema_decay") is not None) != (fc["ema"] is not None):
            return None
        ps = [p for p in group["params"] if p.grad is not None]
        if len(ps) != len(fc["ps"]) or any(a is not b for a, b in zip(ps, fc["ps"])):
            return None
        arr = fc["arr"]
        for i, p in enumerate(ps):
            g = p.grad
            if g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous() or g.device != p.device:
                raise HkpError("FusedAdam: fp32 contiguous CUDA gradients only")
            arr[i].grad = g.data_ptr()
        return fc

    def _fast_launch(self, group, fc, coef):
        torch._foreach_add_(fc["steps"], 1.0)
        fc["step"] += 1
        self._launch(group, fc["ps"], fc["arr"], fc["step"], coef, fc["ema"])

    def _launch(self, group, ps, arr, step, coef=None, ema=None):
        b1, b2 = group["betas"]
        bc1 = 1.0 - b1 ** step
        bc2 = 1.0 - b2 ** step
        stream = ctypes.c_void_p(torch.cuda.current_stream(ps[0].device).cuda_stream)
        moved = ps + [self.state[p][k] for p in ps for k in ("exp_avg", "exp_avg_sq")]
        if coef is None and ema is None:
            call("hkp_adam_step", len(ps), arr, b2, 1.0 - b1, 1.0 - b2, group["eps"], group["weight_decay"],
                 -group["lr"] / bc1, math.sqrt(bc2), stream)
        else:
            omd = 1.0 - group["ema_decay"] if ema is not None else 0.0
            call("hkp_adam_step_ex", len(ps), arr, ema, omd, coef, b2, 1.0 - b1, 1.0 - b2, group["eps"],
                 group["weight_decay"], -group["lr"] / bc1, math.sqrt(bc2), stream)
            if ema is not None:
                moved = moved + [self.state[p]["ema"] for p in ps]
        # the kernel wrote p, exp_avg, exp_avg_sq behind autograd's back: bump
        # their version counters as torch's in-place Adam ops do (operand caches
        # keyed on the version — the packed conv weights — see the change)
        torch.autograd.graph.increment_version(moved)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        max_norm = self._max_grad_norm()
        tables = {}
        clipped = False
        if max_norm is not None:
            if len(self.param_groups) == 1:       # one group on its fast path: the step's table serves the norm
                fc = self._fast_table(0, self.param_groups[0])
                if fc is not None and fc["ps"]:
                    tables[0] = fc
                    self._norm_launch(fc["arr"], fc["ps"], max_norm)
                    clipped = True
            if not clipped:
                clipped = self._grad_norm(max_norm)
        for gi, group in enumerate(self.param_groups):
            coef = None
            if clipped and group.get("max_grad_norm") is not None:
                coef = ctypes.c_void_p(self._norm_out.data_ptr() + 4)
            fc = tables.get(gi) or self._fast_table(gi, group)
            if fc is not None:
                self._fast_launch(group, fc, coef)
                continue
            self._fast.pop(gi, None)
            want_ema = group.get("ema_decay") is not None
            # one launch set per distinct step count (all equal in practice)
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.dtype != torch.float32 or p.device.type != "cuda" or p.grad.dtype != torch.float32:
                    raise HkpError("FusedAdam: fp32 CUDA parameters and gradients only")
                if p.grad.is_sparse:
                    raise HkpError("FusedAdam: sparse gradients are not supported")
                st = self.state[p]
                if "step" not in st:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                checked = [(p, "param"), (p.grad, "grad"), (st["exp_avg"], "exp_avg"), (st["exp_avg_sq"], "exp_avg_sq")]
                if want_ema:
                    checked.append((self._ema_of(p), "ema"))
                for t, name in checked:
                    if not t.is_contiguous():
                        raise HkpError("FusedAdam: %s must be contiguous" % name)
                st["step"] += 1
                by_step.setdefault(int(st["step"].item()), []).append(p)
            for step, ps in by_step.items():
                arr = (AdamTensor * len(ps))()
                ema = (ctypes.c_void_p * len(ps))() if want_ema else None
                for i, p in enumerate(ps):
                    st = self.state[p]
                    arr[i].param, arr[i].grad = p.data_ptr(), p.grad.data_ptr()
                    arr[i].exp_avg, arr[i].exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                    arr[i].n = p.numel()
                    if want_ema:
                        ema[i] = st["ema"].data_ptr()
                self._launch(group, ps, arr, step, coef, ema)
                if len(by_step) == 1:      # every parameter of the group at one step count: cacheable
                    self._fast[gi] = dict(ps=ps, arr=arr, step=step, steps=[self.state[p]["step"] for p in ps],
                                          ema=ema)
        return loss
