"""numpy float32 restatement of Quantization_int8Op (operator_cxx/contrib/quantization_int8-inl.h:144-220 forward,
:260-290 backward).  The operator cannot be compiled against the oracle's shim (it needs broadcast::Reduce,
ConfigReduce and control_flow_op.h), so this file is the pin: every operation is rounded to float32 separately, in
the reference's order, and the object carries countdown, init and minmax over calls as the Operator object and
its aux state do.  Comparisons against it are bit-exact."""
import numpy as np

F = np.float32
QUANT_LEVEL = 127          # :107


def roundf(x):
    """C roundf on float32: halves away from zero (mshadow_op::round).  np.round is half-to-even and is wrong
    here.  x + 0.5 is exact in float64 for every float32 x with |x| < 2^52 and rounds to x beyond."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.trunc(x64 + np.copysign(0.5, x64)).astype(np.float32)


def clip(x, t):
    """mshadow_op::clip: x > t ? t : (x < -t ? -t : x); a NaN x passes through"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > t, F(t), np.where(x < -t, F(-t), x)).astype(np.float32)


def fake_quant(x, t, is_weight):
    """:189-190 (weights, not clipped) and :216-217 (activations)"""
    t = F(t)
    with np.errstate(all="ignore"):
        u = F(t / F(QUANT_LEVEL))                      # :184 / :213: DType threshold / int QUANT_LEVEL
        c = np.asarray(x, dtype=np.float32) if is_weight else clip(x, t)
        q = (c / u).astype(np.float32)                 # a correctly rounded float32 divide
        return (roundf(q) * u).astype(np.float32)      # a separate rounding


class QuantInt8Ref:
    def __init__(self, is_weight=True, delay_quant=0, ema_decay=0.99, grad_mode="ste", fix_act_scale=False,
                 minmax=0.0):
        self.is_weight, self.fix_act_scale, self.grad_mode = bool(is_weight), bool(fix_act_scale), grad_mode
        self.ema_decay = F(ema_decay)                  # float ema_decay (:70)
        self.countdown, self.init = int(delay_quant), True   # :103-106
        self.minmax = F(minmax)                        # the aux state (INIT_ZERO, or a checkpoint's value)

    @property
    def state(self):
        return [self.countdown, int(self.init)]

    def forward(self, x, is_train=True):
        x = np.asarray(x, dtype=np.float32)
        if is_train and self.countdown > 0:            # :144-147
            self.countdown -= 1
            return x.copy()
        if is_train and not self.fix_act_scale:        # :176 / :193
            m = F(np.max(np.abs(x)))                   # find_max: max(|min|, |max|)
            if self.is_weight:
                self.minmax = m                        # :178
            elif self.init:                            # :196-203
                if float(self.minmax) < 1e-6:          # a float against a double literal
                    self.minmax = m
                self.init = False
            else:                                      # :205-207: two products and a sum, each rounded
                d = self.ema_decay
                o = F(F(1) - d)
                self.minmax = F(F(d * self.minmax) + F(o * m))
        return fake_quant(x, self.minmax, self.is_weight)

    def backward(self, ograd, x):
        ograd = np.asarray(ograd, dtype=np.float32)
        if self.grad_mode == "ste" or self.is_weight:  # :260-262
            return ograd.copy()
        assert self.grad_mode == "clip"                # :263-290
        t = self.minmax
        x = np.asarray(x, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            keep = (x >= -t) & (x <= t)
        return np.where(keep, ograd, F(0)).astype(np.float32)
