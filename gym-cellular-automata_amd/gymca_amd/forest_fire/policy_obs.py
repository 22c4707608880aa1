"""observe() of the batched bulldozer and helicopter envs: a compact policy observation in one launch.

gca_policy_observation reads every env's current plane buf[parity[e]][e] once and writes

    local   uint8   (E, S, S), S = 2 radius + 1: the classes of the cells around the agent (0 other, 1 TREE, 2 FIRE,
            3 outside the grid)
    coarse  float32 (E, 2, Hc, Wc), Hc = ceil(H / block), Wc = ceil(W / block): the TREE and the FIRE cells of every
            block x block tile times 1 / block^2 (exact)

with no gather of the two planes (env.grids()), no allocation (given outputs) and no sync, so an agent loop
observe -> policy -> step stays on the device and can be captured in a graph. One function for both env classes: they
share the fields it reads (buf, parity, pos, the three codes).
"""
from .. import _device as dev
from .._lib import SLOT, BoundCall
from ._batched import check_tensor


def output_shapes(env, radius, block):
    """((E, S, S), (E, 2, Hc, Wc)) of observe(radius, block)."""
    E, H, W = env.num_envs, env.nrows, env.ncols
    S = 2 * radius + 1
    return (E, S, S), (E, 2, -(-H // block), -(-W // block))


def observe(env, radius=16, block=16, local_out=None, coarse_out=None, form=0):
    """(local, coarse) of every env of `env` (see the module docstring), allocated here unless given; given outputs are
    written in place and returned. form: 0 picks the kernel by shape, 1 / 2 force the generic / the rows form
    (include/gca.h). The call is pre-bound per (radius, block, form) with the outputs as per-call values, so one bound
    call serves any output tensors; env.rebind() (which an assignment to env.buf / parity / pos runs by itself) drops
    it."""
    import torch

    radius, block, form = int(radius), int(block), int(form)
    if not 0 <= radius <= 31:
        raise ValueError("observe: radius must be in [0, 31]")
    if not (1 <= block <= 64 and block & (block - 1) == 0):
        raise ValueError("observe: block must be a power of two in [1, 64]")
    if form not in (0, 1, 2):
        raise ValueError("observe: form must be 0 (by shape), 1 (generic) or 2 (rows)")
    ls, cs = output_shapes(env, radius, block)
    local_out = torch.empty(ls, dtype=torch.uint8, device=env.device) if local_out is None else \
        check_tensor(local_out, torch.uint8, ls, env._dev_index, "observe", "local_out")
    coarse_out = torch.empty(cs, dtype=torch.float32, device=env.device) if coarse_out is None else \
        check_tensor(coarse_out, torch.float32, cs, env._dev_index, "observe", "coarse_out")
    calls = env._observe_calls
    key = (radius, block, form)
    oc = calls.get(key)
    if oc is None:
        oc = calls[key] = BoundCall(
            "gca_policy_observation", dev.ptr(env.buf[0]), dev.ptr(env.buf[1]), dev.ptr(env.parity), dev.ptr(env.pos),
            env.num_envs, env.nrows, env.ncols, env._empty, env._tree, env._fire, radius, block, form, SLOT, SLOT, SLOT,
            keep=(env.buf, env.parity, env.pos))
    oc(local_out.data_ptr(), coarse_out.data_ptr(), dev.raw_stream(env._dev_index))
    return local_out, coarse_out
