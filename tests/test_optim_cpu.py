"""Host side of gradient clipping and the weight EMA (no GPU): the argument checks
of hkp_grad_norm / hkp_adam_step_ex before any launch, hkp_grad_norm_partials on
hand-counted tables, and the option checks of FusedAdam, Trainer and config."""
import ctypes

import pytest
import torch


def _table(ns, ptr=16):
    from hkp import _lib
    ts = (_lib.AdamTensor * max(len(ns), 1))()
    for t, n in zip(ts, ns):
        t.param = t.grad = t.exp_avg = t.exp_avg_sq = ptr if n else 0
        t.n = n
    return ts


def test_grad_norm_partials_hand_counted():
    from hkp import _lib
    f = _lib.lib().hkp_grad_norm_partials
    # one partial per started 4096-element unit of each tensor; empty tensors have none
    assert f(0, _table([])) == 0
    assert f(1, _table([0])) == 0
    assert f(1, _table([1])) == 1
    assert f(1, _table([4096])) == 1
    assert f(1, _table([4097])) == 2
    assert f(5, _table([1, 37, 4096, 4097, 3 * 4096 + 5])) == 1 + 1 + 1 + 2 + 4
    assert f(3, _table([300 * 4096 + 1, 0, 8192])) == 301 + 0 + 2
    assert f(50, _table([4097] * 50)) == 100              # past the 48 tensors of one launch
    assert f(1, _table([-1])) == -1 and f(-1, _table([1])) == -1


def test_grad_norm_host_side_errors():
    """Every refusal comes before a launch (the pointers are not device memory)."""
    from hkp import _lib
    ts = _table([8, 4097])
    P = ctypes.c_void_p
    with pytest.raises(_lib.HkpError, match="max_norm"):
        _lib.call("hkp_grad_norm", 2, ts, 0.0, P(16), 3, P(16), None)
    with pytest.raises(_lib.HkpError, match="max_norm"):
        _lib.call("hkp_grad_norm", 2, ts, -1.0, P(16), 3, P(16), None)
    with pytest.raises(_lib.HkpError, match="max_norm"):
        _lib.call("hkp_grad_norm", 2, ts, float("nan"), P(16), 3, P(16), None)
    with pytest.raises(_lib.HkpError, match="null output"):
        _lib.call("hkp_grad_norm", 2, ts, 1.0, P(16), 3, None, None)
    with pytest.raises(_lib.HkpError, match="too small"):
        _lib.call("hkp_grad_norm", 2, ts, 1.0, P(16), 2, P(16), None)        # needs 1 + 2
    with pytest.raises(_lib.HkpError, match="too small"):
        _lib.call("hkp_grad_norm", 2, ts, float("inf"), None, 3, P(16), None)
    with pytest.raises(_lib.HkpError, match="bad tensor list"):
        _lib.call("hkp_grad_norm", 2, None, 1.0, P(16), 3, P(16), None)
    ts[1].grad = 0                                                           # null gradient with n > 0
    with pytest.raises(_lib.HkpError, match="tensor 1: null pointer"):
        _lib.call("hkp_grad_norm", 2, ts, 1.0, P(16), 3, P(16), None)


def test_adam_step_ex_host_side_errors():
    from hkp import _lib
    assert ctypes.sizeof(_lib.AdamTensor) == 40
    P = ctypes.c_void_p
    ts = _table([8, 8])
    ema = (P * 2)(16, 16)
    adam = (0.999, 0.1, 0.001, 1e-8, 0.0, -1e-3)
    for bad in (0.0, 0.5, 0.75, -0.1, float("nan")):
        with pytest.raises(_lib.HkpError, match="one_minus_decay"):
            _lib.call("hkp_adam_step_ex", 2, ts, ema, bad, None, *adam, 1.0, None)
    with pytest.raises(_lib.HkpError, match="bias_correction2_sqrt"):
        _lib.call("hkp_adam_step_ex", 2, ts, ema, 0.1, P(16), *adam, 0.0, None)
    with pytest.raises(_lib.HkpError, match="bias_correction2_sqrt"):       # neither extra: hkp_adam_step's checks
        _lib.call("hkp_adam_step_ex", 2, ts, None, 0.0, None, *adam, 0.0, None)
    ema[1] = None
    with pytest.raises(_lib.HkpError, match="tensor 1: null ema pointer"):
        _lib.call("hkp_adam_step_ex", 2, ts, ema, 0.1, None, *adam, 1.0, None)
    ts[0].exp_avg = 0
    with pytest.raises(_lib.HkpError, match="tensor 0: null pointer"):
        _lib.call("hkp_adam_step_ex", 2, ts, None, 0.0, P(16), *adam, 1.0, None)
    with pytest.raises(_lib.HkpError, match="bad tensor list"):
        _lib.call("hkp_adam_step_ex", 2, None, None, 0.0, P(16), *adam, 1.0, None)
    # nothing to do: no launch, with and without the extras
    assert _lib.call("hkp_adam_step_ex", 0, ts, None, 0.0, P(16), *adam, 1.0, None) == 0
    assert _lib.call("hkp_adam_step_ex", 2, _table([0, 0]), ema, 0.1, P(16), *adam, 1.0, None) == 0


def test_fused_adam_option_checks():
    from hkp.optim import FusedAdam
    p = [torch.nn.Parameter(torch.zeros(4))]
    for bad in (0.5, 0.3, 0.0, 1.0, 1.5, -0.9, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdam(p, ema_decay=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdam(p, max_grad_norm=bad)
    opt = FusedAdam(p, lr=1e-4, max_grad_norm=1.0, ema_decay=0.999)
    assert opt.param_groups[0]["max_grad_norm"] == 1.0 and opt.param_groups[0]["ema_decay"] == 0.999
    assert opt.grad_norm is None and opt.clip_coef is None                  # no step yet
    FusedAdam(p, max_grad_norm=float("inf"))                                # the norm only
    with pytest.raises(ValueError, match="ema_decay"):                      # per group, too
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "ema_decay": 0.5})
    off = FusedAdam(p)
    assert off.param_groups[0]["max_grad_norm"] is None and off.param_groups[0]["ema_decay"] is None
    assert off.ema_parameters() == []
    from hkp._lib import HkpError
    with pytest.raises(HkpError, match="ema_decay"):
        with off.ema_weights():
            pass
    p[0].grad = torch.zeros(4)
    with pytest.raises(HkpError, match="CUDA"):                             # no CPU path for the norm either
        opt.step()
    assert opt.grad_norm is None
    # a torch.optim.Adam state dict (no option keys) leaves this optimizer's options on
    opt.load_state_dict(torch.optim.Adam(p, lr=1e-4).state_dict())
    assert opt.param_groups[0]["max_grad_norm"] == 1.0 and opt.param_groups[0]["ema_decay"] == 0.999
    torch.optim.Adam(p).load_state_dict(opt.state_dict())                   # and the other way


def test_trainer_torch_optimizer_rejects_options():
    from hkp import train
    from src.model import KeypointsGauss
    m = KeypointsGauss(2, backbone="resnet18", pretrained=False)
    with pytest.raises(ValueError, match="fused"):
        train.Trainer(m, optimizer="torch", max_grad_norm=1.0)
    with pytest.raises(ValueError, match="fused"):
        train.Trainer(m, optimizer="torch", ema_decay=0.999)
    t = train.Trainer(m, max_grad_norm=2.0, ema_decay=0.9)
    assert t.opt.param_groups[0]["max_grad_norm"] == 2.0 and t.opt.param_groups[0]["ema_decay"] == 0.9
    assert isinstance(train.Trainer(m, optimizer="torch").opt, torch.optim.Adam)


def test_config_defaults_are_none():
    import config
    import train as train_mod
    assert config.MAX_GRAD_NORM is None and config.EMA_DECAY is None
    assert train_mod.MAX_GRAD_NORM is None and train_mod.EMA_DECAY is None
