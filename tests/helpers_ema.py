"""float64 reference of the averaged-weights recurrence (szn_ema_step, engine.TrainStep ema=) and its error bound.

    avg <- param + D (avg - param),   D = min(decay, (1 + s) / (10 + s)) ^ every   (warmup=False: D = decay ^ every)

s = the optimizer steps APPLIED before this one.  The host launches the update on every `every`-th attempted step; a step the
dynamic loss scale skips neither updates the average nor counts towards s."""
import numpy as np

EPS = 2.0 ** -24          # half an ulp of a float32 in [1, 2): the relative error of one rounding


def ema_factor(decay, every=1, s=0, warmup=True):
    """D as a float64 (the kernel receives decay as a float32 and rounds D to float32 once)"""
    d = float(np.float32(decay))
    if warmup:
        d = min(d, (1.0 + s) / (10.0 + s))
    return d ** int(every)


def _f64(a):
    """numpy arrays (and lists) as float64 arrays; torch tensors as float64 tensors where they live (the engine tests keep their
    135 M-element buffers on the device: the same IEEE double arithmetic, no read-back)"""
    return a.double() if hasattr(a, "double") else np.asarray(a, dtype=np.float64)


def ema_update(avg, param, D):
    avg, param = _f64(avg), _f64(param)
    return param + D * (avg - param)


def ema_step_bound(avg, param):
    """per element: one rounding in avg - param, one in the fmaf, D rounded to float32 -> 4 * 2^-24 * max(|avg|, |param|)"""
    a, p = abs(_f64(avg)), abs(_f64(param))
    return 4.0 * EPS * (a.maximum(p) if hasattr(a, "double") else np.maximum(a, p))


def ema_run(avg0, params, decay, every=1, warmup=True, applied=None):
    """avg0: the average before the first step; params: the parameters after step 1, 2, ...; applied[t]: False = step t + 1 was
    skipped.  -> [(avg after the step, accumulated error bound, D of the step or None, updates so far)]"""
    ref = Recurrence(avg0, decay, every, warmup)
    return [ref.step(p, applied is None or bool(applied[t])) for t, p in enumerate(params)]


class Recurrence(object):
    """the recurrence one step at a time (the engine tests read the parameters back after every training step)"""

    def __init__(self, avg0, decay, every=1, warmup=True):
        self.avg = _f64(avg0)
        self.bound = self.avg * 0.0
        self.decay, self.every, self.warmup = decay, every, warmup
        self.t = self.s = self.updates = 0

    def step(self, param, applied=True):
        """the parameters after one more attempted step -> (avg, accumulated bound, D or None, launches so far)"""
        self.t += 1
        D = None
        if self.t % self.every == 0:
            self.updates += 1                 # the launch happens; the kernel does nothing on a skipped step
            if applied:
                D = ema_factor(self.decay, self.every, self.s, self.warmup)
                self.bound = D * self.bound + ema_step_bound(self.avg, param)
                self.avg = ema_update(self.avg, param, D)
        if applied:
            self.s += 1
        return self.avg, self.bound, D, self.updates
