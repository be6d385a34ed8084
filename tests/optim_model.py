"""numpy float32 models of the Adam and SGD-momentum kernels (csrc/misc.hip: adam_kernel, sgd_kernel), operation by operation, for
tests/test_optim_host.py and tests/test_gpu_optim.py.  Like gradnorm_model.adamw they assume no fused multiply-add anywhere: compare
with a tolerance, or use them for properties.  The host-side scalars (step size, bias correction) are formed in double and rounded
to float32 once, as the entry points do; Adam's betas are doubles there (1.0f - 0.999f is 1.3e-5 off 0.001, which the second moment
would carry: measured at 1.24 of the tests' bound against torch.optim.Adam at gradients of size 15)."""
import math

import numpy as np

f = np.float32


def adam(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale):
    """adam_kernel: single-tensor torch.optim.Adam, no amsgrad, coupled L2 decay.  Returns (p, m, v) as new float32 arrays."""
    p, g, m, v = (np.asarray(a, dtype=f).copy() for a in (p, g, m, v))
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    omb1, omb2 = f(1.0 - float(b1)), f(1.0 - float(b2))       # complements in double from double betas, rounded once
    b1, b2 = f(b1), f(b2)
    step_size, bc2_sqrt = f(float(f(lr)) / bc1), f(math.sqrt(bc2))
    eps, wd, gs = f(eps), f(wd), f(grad_scale)
    gt = g * gs
    if wd > 0:
        gt = gt + wd * p
    m = m * b1 + gt * omb1
    v = v * b2 + gt * gt * omb2
    denom = np.sqrt(v) / bc2_sqrt + eps
    p = p - step_size * (m / denom)
    return p.astype(f), m.astype(f), v.astype(f)


def sgd(p, g, buf, lr, momentum, wd, grad_scale):
    """sgd_kernel: torch.optim.SGD with momentum, dampening 0, no Nesterov.  A zero `buf` is torch's first step (buf = g').  Returns
    (p, buf) as new float32 arrays."""
    p, g, buf = (np.asarray(a, dtype=f).copy() for a in (p, g, buf))
    lr, momentum, wd, gs = f(lr), f(momentum), f(wd), f(grad_scale)
    gt = g * gs
    if wd > 0:
        gt = gt + wd * p
    buf = buf * momentum + gt
    p = p - lr * buf
    return p.astype(f), buf.astype(f)

