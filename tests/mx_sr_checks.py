"""What the stochastic-rounding tests of the MXFP4 gradient quantisers share
(``test_mxfp4_sr_cpu.py``, ``test_gpu_mxfp4_sr.py``): the reference images, the
gradient products of the bias measurement and the tiny-model run.  A plain
helper module, not collected."""
import torch

import mx_linear_checks as lc
from mxk8s.models.llama import Llama, LlamaConfig
from mxk8s.ops.mxfp4 import (dequantize_mxfp4, quantize_mxfp4_ref, sr_reseed)

M64 = 2 ** 64
SEEDS = [0, 1, M64 - 1, 0x9E3779B97F4A7C15]
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def ref(x, seed=None):
    """Reference images of x (any device, made contiguous on the CPU)."""
    x = x.cpu().contiguous()
    return quantize_mxfp4_ref(x) if seed is None else quantize_mxfp4_ref(x, "stochastic", seed)


def deq(pair):
    return dequantize_mxfp4(*pair).double()


def noclip_scales(x):
    """The scale bytes of the non-clipping rule, from first principles: the
    smallest e >= -127 with amax 2^-e <= 6 that the OCP exponent or its
    successor gives; 127 for a zero block."""
    R, K = x.shape
    amax = x.double().abs().reshape(R, K // 32, 32).amax(dim=2)
    e = torch.floor(torch.log2(torch.where(amax > 0, amax, torch.ones_like(amax)))).to(torch.int64) - 2
    e = e.clamp(-127, 127)
    e = e + (torch.ldexp(amax, -e) > 6).to(torch.int64)
    return torch.where(amax > 0, e + 127, torch.full_like(e, 127)).to(torch.uint8)


def grid_tensor(R, K, seed):
    """bf16 [R, K] (multiples of 32) on the MX grid along both axes: every value
    an e2m1 magnitude times the power of two of its 32 x 32 tile, whose diagonal
    holds a 4 or a 6, so that every row block and every column block has that
    power as its scale under either rounding."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randint(0, 8, (R // 32, 32, K // 32, 32), generator=g)
    d = torch.arange(32)
    code[:, d, :, d] = 6 + torch.randint(0, 2, (32, R // 32, K // 32), generator=g)
    sign = torch.randint(0, 2, code.shape, generator=g) * 2 - 1
    e = torch.randint(-20, 20, (R // 32, 1, K // 32, 1), generator=g)
    x = torch.ldexp(torch.tensor(E2M1)[code] * sign, e).reshape(R, K)
    return x.bfloat16()


def gradient_errors(T, i, o, seed, sr_seeds):
    """dx and dW of linear_mxfp4's backward from reference images, in fp64,
    against the products with an unquantised dy: {name: (RNE error norm, error
    norm of the mean of the stochastic draws, RNE projection, mean's projection)},
    the projections those of the error on the true product."""
    x, w, dy = lc.operands(T, i, o, seed)
    wt, xt = deq(ref(w.t())), deq(ref(x.t()))                 # [in, out], [in, T]: round-to-nearest
    true = {"dx": dy.double() @ wt.t(), "dw": dy.double().t() @ xt.t()}

    def grads(s):
        rows = ref(dy, s)
        cols = ref(dy.t(), None if s is None else (s + 1) % M64)
        return {"dx": deq(rows) @ wt.t(), "dw": deq(cols) @ xt.t()}

    rne = grads(None)
    draws = [grads(s) for s in sr_seeds]
    out = {}
    for k, t in true.items():
        mean = sum(d[k] for d in draws) / len(draws)
        proj = lambda g: (((g - t) * t).sum() / (t * t).sum()).item()   # noqa: E731
        out[k] = ((rne[k] - t).norm().item(), (mean - t).norm().item(), proj(rne[k]), proj(mean))
    return out


def sr_model_run(ref_model, tok, dev, grad_rounding, sr_seed=0):
    """The tiny Llama with MXFP4 linears on ``dev`` (bf16 there, fp32 on the
    CPU), weights of ``ref_model``, one forward + backward: (model, loss)."""
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype = "mxfp4"
    cfg.grad_rounding = grad_rounding
    m = Llama(cfg)
    m.load_state_dict(ref_model.state_dict())
    if torch.device(dev).type != "cpu":
        m = m.to(dev, torch.bfloat16)
    sr_reseed(sr_seed)
    loss = m.loss(tok.to(dev))
    loss.backward()
    return m, loss


def min_cosine(ref_model, model):
    worst = 1.0
    for (n, pr), (_, pm) in zip(ref_model.named_parameters(), model.named_parameters()):
        a, b = pr.grad.double().flatten(), pm.grad.double().cpu().flatten()
        assert torch.isfinite(b).all(), n
        cos = (a @ b / (a.norm() * b.norm())).item()
        print(n, round(cos, 5))
        worst = min(worst, cos)
    return worst
