"""Plain fp64 restatement of a text query's steps 3-5: text features -> centre row -> text_projection -> query
code and its bits, with a DERIVED per-element error bound, an fp32 emulation in another summation order with switchable deliberate
defects, and the seeded inputs that tests/test_text_query_cpu.py (CPU) and tests/test_text_query_gpu.py (GPU) share.  Nothing is tuned
to a measured error; the vocabulary (U32, gam(p), TINY, breaches) is that of tests/train_kernels_ref.py and the one-layer term is
tests/forward_kernels_ref.py's `small_linear_ref`, the restatement of the kernel both the load-time fold and ch_model_project_text launch.

The bound
=========
  step 3  c = sign(f): exact (+-1, or 0 for an exact zero), so the first layer's operand carries no error.
  step 4  one Linear y = W c + b through small_linear_kernel: a lane adds ceil(cd / 64) products one after the other, the wave sum adds 6
          butterfly steps, then the bias: p = ceil(cd / 64) + 8 roundings (the product included), |error| <= gam(p) (|W| |c| + |b|).
          Sequential(Linear, ReLU, Linear): h = relu(W0 c + b0) with e_h = gam(p) (|W0| |c| + |b0|) (ReLU is exact and 1-Lipschitz), then
          z = W2 h' + b2 on the fp32 h' the kernel holds, |h' - h| <= e_h:
              |error| <= |W2| e_h + gam(p) (|W2| (|h| + e_h) + |b2|).
  step 5  the query code is z itself; bit j = z_j > 0 (pack_sign).  A bit may differ from the fp64 one only where |z_j| <= bound_j.

Defects (each must leave the bound at every shape it applies to, or the bound shows nothing):
  bias_dropped        the output layer's bias is not added
  weight_transposed   the output layer's weight [nbit, cd] is read as if stored [cd, nbit]
  wrong_prompt        row r gets the cd features of prompt r + 1 (N > 1 only: one prompt has no neighbour)
  relu_missing        (two layers) the first layer's activation flag is off
  hidden_unactivated  (two layers) the second layer is fed the buffer in front of the first layer's launch -- the centre rows themselves,
                      which have the hidden rows' width -- so nothing of the first layer, activation included, reaches it
"""
import torch

from forward_kernels_ref import cdiv, small_linear_ref
from train_kernels_ref import TINY, breaches, gam, gen as _tr_gen  # noqa: F401  (breaches: re-exported for the two test files)

CENTER_DIMS = (64, 512)
NBITS = (12, 64, 128)              # a partly filled word, one word, two words
NS = (1, 3, 257)
FORMS = ("linear", "mlp")          # Linear | Sequential(Linear, ReLU, Linear)
DEFECTS = {"linear": ("bias_dropped", "weight_transposed", "wrong_prompt"),
           "mlp": ("bias_dropped", "weight_transposed", "wrong_prompt", "relu_missing", "hidden_unactivated")}


def gen(name, *key):
    return _tr_gen("text_query/" + name, *key)


def projection_weights(cd, nbit, form):
    """text_projection in the state_dict layout of the form: N(0, 1 / fan_in) weights, N(0, 1) biases (a dropped bias is then visible)"""
    g = gen("weights", cd, nbit, form)

    def lin(out_f):
        return torch.randn(out_f, cd, generator=g) * cd ** -0.5, torch.randn(out_f, generator=g)
    if form == "linear":
        w, b = lin(nbit)
        return {"text_projection.weight": w, "text_projection.bias": b}
    w0, b0 = lin(cd)
    w2, b2 = lin(nbit)
    return {"text_projection.0.weight": w0, "text_projection.0.bias": b0, "text_projection.2.weight": w2, "text_projection.2.bias": b2}


def features(N, cd):
    """[N, cd] fp32 stand-ins for pooler_output rows; every 17th entry is an exact zero (sign(0) = 0 must stay 0)"""
    f = torch.randn(N, cd, generator=gen("features", N, cd))
    f.view(-1)[::17] = 0.0
    return f


def centre_rows(f):
    """step 3 through the code the codebook builder runs"""
    from trainers.orthohash import centre_rows as rows
    return rows(f)


def _layers(sd):
    if "text_projection.weight" in sd:
        return None, (sd["text_projection.weight"], sd["text_projection.bias"])
    return (sd["text_projection.0.weight"], sd["text_projection.0.bias"]), (sd["text_projection.2.weight"], sd["text_projection.2.bias"])


def text_query_ref(f, sd):
    """f [N, cd] fp32 text features, sd: text_projection.* -> (z [N, nbit] fp64, bound [N, nbit] fp64)"""
    first, (w, b) = _layers(sd)
    c = centre_rows(f)
    assert bool(((c == 0) == (f == 0)).all()) and bool((c.abs() <= 1).all())
    if first is None:
        return small_linear_ref(c, w, b, 0)
    h, e_h = small_linear_ref(c, first[0], first[1], 1)
    wd, bd = w.double(), b.double()
    z = h @ wd.t() + bd
    p = cdiv(h.shape[1], 64) + 8
    return z, e_h @ wd.abs().t() + gam(p) * ((h.abs() + e_h) @ wd.abs().t() + bd.abs()) + TINY


def text_query_bits(z):
    """step 5: the packed bits as booleans [N, nbit] (pack_sign: strictly positive)"""
    return z > 0


def text_query_emul(f, sd, defect=None):
    """fp32, torch's matmul on the flipped operands (another summation order than the kernel's), with one named defect or none"""
    first, (w, b) = _layers(sd)
    c = centre_rows(f)
    if defect == "wrong_prompt":
        c = c.roll(-1, 0)

    def linear(x, W, bias):
        return x.flip(1) @ W.flip(1).t() + bias
    x = c
    if first is not None and defect != "hidden_unactivated":
        x = linear(c, first[0], first[1])
        if defect != "relu_missing":
            x = x.clamp_min(0)
    if defect == "weight_transposed":
        w = w.t().contiguous().view(w.shape)
    z = linear(x, w, b)
    return z - b if defect == "bias_dropped" else z


def flips_are_inside_the_bound(got, z, bound):
    """every sign bit of `got` that differs from the fp64 one belongs to an entry whose fp64 magnitude is below its bound"""
    diff = text_query_bits(got.double()) != text_query_bits(z)
    return bool((z.abs()[diff] <= bound[diff]).all()), int(diff.sum())
