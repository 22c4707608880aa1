"""Yardsticks of the optimizer (include/gca.h "optimizer"): gca_adam_step restated in numpy, one rounded float32
operation at a time in the header's order (the definition the device kernels and the host build are held against, bit
for bit); gca_permutation restated on oracle.philox; optax's clip_by_global_norm and adam with the reference's
linear_schedule restated in float64 from their published formulas (the accuracy yardstick); the shared cases and the
driver of either build. Test infrastructure only: the product never imports it."""
import numpy as np

from oracle import philox

f32 = np.float32
TAG_PERM = 0x5045524D
LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025, 70001)   # mixed in one call: tails of every kind, several chunks
PERM_SIZES = list(range(1, 513)) + [1000, 4099, 65537]   # 3 rows each
HYPER = dict(lr=2.5e-4, b1=0.9, b2=0.999, eps=1e-5, max_grad_norm=0.5, anneal=None)


# ------------------------------------------------------------------ gca_adam_step in float32, the header's order
def chunk(total):
    return 1024 * max(1, -(-total // (2048 * 1024)))


def _tree(s):
    s = s.copy()
    h = 128
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


def sum_squares(grads):
    """The double sum under the norm: lanes, chunks, trees. Absent elements are +0.0 addends, which change nothing."""
    CH = chunk(sum(g.size for g in grads))
    parts = []
    for g in grads:
        g = g.reshape(-1)
        for base in range(0, g.size, CH):
            c = g[base:base + CH].astype(np.float64)
            sq = np.zeros(-(-c.size // 1024) * 1024)
            sq[:c.size] = c * c
            sq = sq.reshape(-1, 256, 4)
            s = np.zeros(256)
            for k in range(sq.shape[0]):
                for j in range(4):
                    s = s + sq[k, :, j]
            parts.append(_tree(s))
    p = np.zeros(-(-len(parts) // 256) * 256)
    p[:len(parts)] = parts
    s = np.zeros(256)
    for row in p.reshape(-1, 256):
        s = s + row
    return _tree(s)


def lr_at(lr0, count_before, anneal):
    if anneal is None:
        return f32(lr0)
    spi, ni = anneal
    frac = 1.0 - ((count_before // spi) / ni)
    return f32(float(f32(lr0)) * max(frac, 0.0))


class AdamRef:
    """The state and the step of gca_adam_step on lists of float32 arrays."""

    def __init__(self, params, lr=2.5e-4, b1=0.9, b2=0.999, eps=1e-5, max_grad_norm=0.5, anneal=None):
        self.w = [np.array(p, f32) for p in params]
        self.m = [np.zeros_like(p) for p in self.w]
        self.v = [np.zeros_like(p) for p in self.w]
        self.lr0, self.b1, self.b2, self.eps, self.max_norm = f32(lr), f32(b1), f32(b2), f32(eps), f32(max_grad_norm)
        self.anneal = anneal
        self.count, self.b1_pow, self.b2_pow = 0, f32(1), f32(1)

    def step(self, grads):
        one = f32(1)
        lr = lr_at(self.lr0, self.count, self.anneal)
        self.count += 1
        self.b1_pow = f32(self.b1_pow * self.b1)
        self.b2_pow = f32(self.b2_pow * self.b2)
        norm = np.sqrt(f32(sum_squares(grads)))
        assert norm.dtype == f32
        clip = self.max_norm > 0 and not norm < self.max_norm
        omb1, omb2, c1, c2 = one - self.b1, one - self.b2, one - self.b1_pow, one - self.b2_pow
        with np.errstate(all="ignore"):
            for i, g in enumerate(grads):
                g = np.asarray(g, f32)
                gc = (g / norm) * self.max_norm if clip else g
                self.m[i] = (self.b1 * self.m[i]) + (omb1 * gc)
                self.v[i] = (self.b2 * self.v[i]) + ((omb2 * gc) * gc)
                mhat, vhat = self.m[i] / c1, self.v[i] / c2
                self.w[i] = self.w[i] - (lr * (mhat / (np.sqrt(vhat) + self.eps)))
                assert self.w[i].dtype == f32 and self.m[i].dtype == f32 and self.v[i].dtype == f32
        return norm, lr


# ------------------------------------------------------------------ optax in float64
class OptaxRef:
    """optax.chain(clip_by_global_norm(max_norm), adam(lr, b1, b2, eps)) in float64 from the published formulas:
    g' = g if norm < max_norm else (g / norm) * max_norm; mu = b1 mu + (1 - b1) g'; nu = b2 nu + (1 - b2) g'^2;
    update = -lr (mu / (1 - b1^t)) / (sqrt(nu / (1 - b2^t)) + eps); lr = the reference's linear_schedule(count)."""

    def __init__(self, params, lr=2.5e-4, b1=0.9, b2=0.999, eps=1e-5, max_grad_norm=0.5, anneal=None):
        self.w = [np.array(p, np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.w]
        self.v = [np.zeros_like(p) for p in self.w]
        self.lr0, self.b1, self.b2, self.eps, self.max_norm = (float(f32(x)) for x in (lr, b1, b2, eps, max_grad_norm))
        self.anneal, self.count = anneal, 0

    def step(self, grads):
        lr = self.lr0
        if self.anneal is not None:
            lr = self.lr0 * max(1.0 - (self.count // self.anneal[0]) / self.anneal[1], 0.0)
        self.count += 1
        grads = [np.asarray(g, np.float64) for g in grads]
        norm = np.sqrt(sum(float((g * g).sum()) for g in grads))
        if self.max_norm > 0 and not norm < self.max_norm:
            grads = [(g / norm) * self.max_norm for g in grads]
        for i, g in enumerate(grads):
            self.m[i] = self.b1 * self.m[i] + (1 - self.b1) * g
            self.v[i] = self.b2 * self.v[i] + (1 - self.b2) * g * g
            mhat, vhat = self.m[i] / (1 - self.b1 ** self.count), self.v[i] / (1 - self.b2 ** self.count)
            self.w[i] = self.w[i] - lr * mhat / (np.sqrt(vhat) + self.eps)
        return norm, lr


def torch_f32_adam(params, grad_steps, lr=2.5e-4, b1=0.9, b2=0.999, eps=1e-5, max_grad_norm=0.5):
    """The same steps in plain torch float32 ops (the formulation a user would write): the tolerance's yardstick."""
    import torch

    w = [torch.tensor(np.asarray(p, f32)) for p in params]
    m, v = [torch.zeros_like(p) for p in w], [torch.zeros_like(p) for p in w]
    for t, grads in enumerate(grad_steps, 1):
        g = [torch.tensor(np.asarray(x, f32)) for x in grads]
        norm = torch.sqrt(sum((x * x).sum() for x in g))
        if max_grad_norm > 0 and not norm < max_grad_norm:
            g = [x / norm * max_grad_norm for x in g]
        for i, x in enumerate(g):
            m[i].mul_(b1).add_(x, alpha=1 - b1)
            v[i].mul_(b2).addcmul_(x, x, value=1 - b2)
            denom = (v[i] / (1 - b2 ** t)).sqrt_().add_(eps)
            w[i].addcdiv_(m[i], denom, value=-lr / (1 - b1 ** t))
    return [x.numpy() for x in w]


# ------------------------------------------------------------------ cases
def tensors(lengths=LENGTHS, seed=0):
    """[w] float32: both signs, magnitudes over a few decades."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 0, n)).astype(f32) for n in lengths]


def gradients(lengths=LENGTHS, steps=10, seed=1, scale=1.0):
    """steps x [g]: global norms on both sides of 0.5 across the steps when scale = 1 (the scale halves every second
    step from about 3 x 0.5 down), exact zeros and a denormal among the elements."""
    rng = np.random.default_rng(seed)
    total = sum(lengths)
    out = []
    for s in range(steps):
        target = scale * 1.5 * 0.5 ** (s // 2)
        gs = [(rng.standard_normal(n) * target / np.sqrt(total)).astype(f32) for n in lengths]
        gs[-1][::7] = 0
        gs[-1][1] = f32(1e-42)
        out.append(gs)
    return out


# ------------------------------------------------------------------ either build through the public class
def make_opt(params, device="cpu", offset=0, **hyper):
    """(Adam, {name: tensor}): parameter i lives at element `offset` of its own storage (offset = 1: 4-byte aligned
    only, the scalar path)."""
    import torch

    from gymca_amd.forest_fire import ppo

    ps = {}
    for i, p in enumerate(params):
        buf = torch.zeros(p.size + offset, dtype=torch.float32, device=device)
        t = buf[offset:]
        t.copy_(torch.from_numpy(np.ascontiguousarray(p)))
        ps[f"p{i}"] = t
    return ppo.Adam(ps, **hyper), ps


def grads_on(grads, device="cpu", offset=0):
    import torch

    out = {}
    for i, g in enumerate(grads):
        buf = torch.zeros(g.size + offset, dtype=torch.float32, device=device)
        buf[offset:].copy_(torch.from_numpy(np.ascontiguousarray(g)))
        out[f"p{i}"] = buf[offset:]
    return out


def bits(a):
    import torch

    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def opt_state(opt):
    """(count, b1_pow, b2_pow, norm, lr) read back from the state block."""
    s = opt.state.cpu().numpy()
    fl = s.view(f32)
    return int(s[0]), fl[1], fl[2], fl[3], fl[4]


# ------------------------------------------------------------------ gca_permutation
def half_bits(T):
    h = 1
    while (1 << (2 * h)) < T:
        h += 1
    return h


def permutation_ref(T, rows, seed, epoch0=0, counter=0):
    """(out int32 (rows, T), the longest walk): the keyed Feistel network of gca.h walked until the value is below T."""
    key = philox.seed_key(seed)
    h = half_bits(T)
    mask = np.uint64((1 << h) - 1)
    # all rows walk together: element (r, i) at flat position r * T + i
    keys = np.repeat((epoch0 + np.arange(rows) + counter) & 0xFFFFFFFF, T).astype(np.uint64)
    x = np.tile(np.arange(T, dtype=np.uint64), rows)
    todo = np.arange(rows * T)
    walks = 0
    while todo.size:
        walks += 1
        assert walks <= 1024, "the walk reached its cap"
        y, k = x[todo], keys[todo]
        L, R = y >> np.uint64(h), y & mask
        for rnd in range(4):
            ctr = np.stack([R, np.full_like(R, rnd), k, np.full_like(R, TAG_PERM)], -1)
            F = philox.philox4x32_10(ctr, key)[:, 0].astype(np.uint64) & mask
            L, R = R, L ^ F
        y = (L << np.uint64(h)) | R
        x[todo] = y
        todo = todo[y >= T]
    return x.astype(np.int32).reshape(rows, T), walks


# ------------------------------------------------------------------ drivers shared by the CPU and the GPU tests
def run_steps(device, ws, grad_steps, offset=0, **hyper):
    """The steps through forest_fire.ppo.Adam on `device`: (opt, params dict, info rows float32 (steps, 2))."""
    import torch

    opt, ps = make_opt(ws, device=device, offset=offset, **hyper)
    info = torch.full((len(grad_steps), 2), float("nan"), device=device)
    for s, g in enumerate(grad_steps):
        got = opt.step(grads_on(g, device=device, offset=offset), info_out=info[s])
        assert got.data_ptr() == info[s].data_ptr()
    return opt, ps, info.cpu().numpy()


def assert_equals_ref(opt, ps, info, ref, norms_lrs, where):
    """Bit for bit: the weights, both moments, the state block's scalars and the info rows."""
    for i in range(len(ref.w)):
        n = f"p{i}"
        assert np.array_equal(bits(ps[n]), bits(ref.w[i])), (where, "w", i)
        assert np.array_equal(bits(opt.m[n]), bits(ref.m[i])), (where, "m", i)
        assert np.array_equal(bits(opt.v[n]), bits(ref.v[i])), (where, "v", i)
    count, b1p, b2p, norm, lr = opt_state(opt)
    assert count == ref.count and bits(b1p) == bits(ref.b1_pow) and bits(b2p) == bits(ref.b2_pow), where
    assert bits(norm) == bits(norms_lrs[-1][0]) and bits(lr) == bits(norms_lrs[-1][1]), where
    assert np.array_equal(bits(info), bits(np.array(norms_lrs, f32))), where


def raw_call(lib_call, n=2, length=5, **over):
    """gca_adam_step of either build through `lib_call(name, *args)` on valid arguments but for `over`; every call the
    tests make with it is refused by an argument check, so no pointer is dereferenced. Keys: t (None: a null table),
    n, len0, w0 / g0 / m0 / v0 (addresses of tensor 0), state, info, ws, ws_bytes, b1, b2, eps, spi, ni."""
    import ctypes

    from gymca_amd import _lib

    t = _lib.AdamTensors()
    t.n = over.get("n", n)
    for i in range(min(max(t.n, 0), 8)):
        t.len[i] = length
        t.w[i], t.g[i], t.m[i], t.v[i] = (0x10000 + 0x1000 * i + 0x100 * k for k in range(4))
    if "len0" in over:
        t.len[0] = over["len0"]
    for k in "wgmv":
        if k + "0" in over:
            getattr(t, k)[0] = over[k + "0"]
    need = 8 * (n * length // 1024 + 8)
    return lib_call("gca_adam_step", None if over.get("t", 1) is None else ctypes.byref(t), over.get("state", 0x20000),
                    2.5e-4, over.get("b1", 0.9), over.get("b2", 0.999), over.get("eps", 1e-5), 0.5,
                    over.get("spi", 0), over.get("ni", 0), over.get("info", None), over.get("ws", 0x30000),
                    over.get("ws_bytes", need), None)
