"""A hot parity case in which every heat ring and the dousing term decide. The marching step's other parity tests run
states where the dousing term exceeds the heat (every probability clamps to 0) or whose outer ring weights are zero,
so a draw almost never lands between a right and a wrong probability. Here heat_dw[k] = 0.25 / (0.3 R (2k+1)^2) for
k = 1..R (every ring contributes the same expected heat at 30 % FIRE), dous_inner = 0.2, dous_border = 0.05 and 2 %
dousing: the C oracle burns between 0.2 and 0.8 of the TREEs with a burning neighbour (asserted, from the oracle
alone), so the f32 heat chain, the layer products and the draw comparison are exercised on tens of thousands of cells.

gca_alex_step_march in its three terrain modes (edge_slope given; edge_slope = NULL; vd = NULL as well), with and
without growth, R = 1..8 at W = 256, R = 7 at 512, R = 8 at 1024: eight different rng_step values from the same state
(the same probabilities under fresh draws) and then a second chained step are bit for bit -- grid, ages, counts --
the C oracle (unit p_slope for the flat modes, the planes of the same altitude for the general one) and
gca_alex_step_packed."""
import numpy as np
import pytest

from alex_cases import make_case
from oracle import alex_c
from test_gpu_alex_draws import _groups_with_multi
from test_gpu_alex_march import _coalesced, _layers, _run, _with_radius
from test_gpu_edge_slope import altitude, params, slopes

pytestmark = pytest.mark.gpu

E, H = 3, 32
UNIFORM = (4, 2)


def balanced_params(R, p_tree, seed):
    p = _with_radius(params(H, p_tree, seed=seed), R)
    for k in range(9):
        p.heat_dw[k] = 0.25 / (R * 0.3 * (2 * k + 1) ** 2) if 1 <= k <= R else 0.0
    p.dous_inner, p.dous_border = 0.2, 0.05
    return p


def balanced_case(W, seed, uniform):
    case = make_case(E, H, W, seed, fire_p=0.3, dousing_p=0.02)
    if uniform:
        case["veg"][...], case["den"][...] = UNIFORM
    return case


def burn_share(g_in, g_out):
    """New fires / TREEs with a burning neighbour."""
    f = np.pad(g_in == 2, ((0, 0), (1, 1), (1, 1)))
    near = np.zeros(g_in.shape, bool)
    for dr in range(3):
        for dc in range(3):
            near |= f[:, dr:dr + g_in.shape[1], dc:dc + g_in.shape[2]]
    probed = (g_in == 1) & near
    return float(((g_out == 2) & probed).sum()) / float(probed.sum())


@pytest.mark.parametrize("p_tree", [0.0, 0.02])
@pytest.mark.parametrize("mode", ["general", "flat", "uniform"])
@pytest.mark.parametrize("W,R", [(256, R) for R in range(1, 9)] + [(512, 7), (1024, 8)])
def test_balanced_hot_state_vs_oracle_and_packed(device, W, R, mode, p_tree):
    import torch

    seed = 300 + R + W
    p = balanced_params(R, p_tree, seed)
    case = balanced_case(W, seed, mode == "uniform")
    if mode == "uniform":
        p.vd_uniform = UNIFORM[0] | UNIFORM[1] << 4
    vd, bits = _layers(device, case)
    if mode == "general":
        es, ps = slopes(device, altitude(E, H, W, seed))
        planes = ps.cpu().numpy()
    else:
        es = None
        planes = np.ones((E, 8, H, W), np.float32)
    coal = _coalesced(device, es if es is not None else torch.ones((E, 4, H, W), dtype=torch.float32, device=device))
    vd_arg = None if mode == "uniform" else vd
    g_in = case["grid"]
    first = None
    for s in [3 + 17 * i for i in range(8)] + [1000]:
        rs = np.full(E, s, np.uint32)
        if s == 1000:  # the second, chained step: from the first launch's output
            case["grid"], case["age"] = first
        want = alex_c.alex_step(p, case["grid"], case["age"], case["veg"], case["den"], case["dous"], planes,
                                case["widx"], rng_step=rs)[:3]
        got = _run(device, "gca_alex_step_march", p, case, es, rs, vd_arg, bits)[:3]
        ref = _run(device, "gca_alex_step_packed", p, case, coal, rs, vd, bits)[:3]
        for name, g, w, t in zip(("grid", "ages", "counts"), got, want, ref):
            assert np.array_equal(g, w), f"march vs oracle, rng_step {s}, {name}: {np.argwhere(g != w)[:5]}"
            assert np.array_equal(g, t), f"march vs packed, rng_step {s}, {name}: {np.argwhere(g != t)[:5]}"
        if s != 1000:
            share = burn_share(g_in, want[0])
            assert 0.2 <= share <= 0.8, share
            multi = _groups_with_multi(g_in, want[0])
            assert multi >= 100, multi
        if first is None:
            first = (want[0], want[1])
