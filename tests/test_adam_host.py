"""CPU: the optimizer and the minibatch shuffle of the PPO update on the host build. gca_adam_step through
forest_fire.ppo.Adam against the float32 restatement of tests/_adam_ref.py bit for bit (mixed lengths, 4-byte-aligned
tensors, clipping on and off, zero gradients, annealing across a boundary and past the end), against optax restated in
float64 within 4 x plain torch float32's error, state_dict round trips; gca_permutation against its restatement for every
small T; every argument error of both entry points with its message, in both builds (the checks run before any
launch, so the device library needs no GPU for them)."""
import ctypes

import numpy as np
import pytest

import _adam_ref as A
import _ppo_ref as R


def _ref_steps(ws, grad_steps, **hyper):
    ref = A.AdamRef(ws, **hyper)
    return ref, [ref.step(g) for g in grad_steps]


@pytest.mark.parametrize("offset", [0, 1])
def test_adam_equals_the_restatement_bit_for_bit(offset):
    ws, gs = A.tensors(), A.gradients()
    ref, nl = _ref_steps(ws, gs, **A.HYPER)
    norms = [float(n) for n, _ in nl]
    assert max(norms) > 0.5 > min(norms)  # both sides of the clip
    opt, ps, info = A.run_steps("cpu", ws, gs, offset=offset, **A.HYPER)
    assert all(p.storage_offset() == offset for p in ps.values())
    A.assert_equals_ref(opt, ps, info, ref, nl, f"offset {offset}")


def test_adam_clipping_cases():
    import torch

    ws = A.tensors()
    # below max_norm: the clip is the identity, bit for bit max_grad_norm = 0
    small = A.gradients(steps=3, scale=0.1)
    hyper = dict(A.HYPER)
    a, pa, ia = A.run_steps("cpu", ws, small, **hyper)
    hyper["max_grad_norm"] = 0.0
    b, pb, ib = A.run_steps("cpu", ws, small, **hyper)
    assert (ia[:, 0] < 0.5).all() and np.array_equal(A.bits(ia), A.bits(ib))  # the norm is recorded without clipping
    assert all(np.array_equal(A.bits(pa[n]), A.bits(pb[n])) for n in pa)
    # above max_norm: the update differs from the unclipped one and equals the restatement
    big = A.gradients(steps=3, scale=4.0)
    ref, nl = _ref_steps(ws, big, **A.HYPER)
    c, pc, ic = A.run_steps("cpu", ws, big, **A.HYPER)
    assert (ic[:, 0] > 0.5).all()
    A.assert_equals_ref(c, pc, ic, ref, nl, "above max_norm")
    d, pd, _ = A.run_steps("cpu", ws, big, **hyper)
    assert not np.array_equal(A.bits(c.m["p7"]), A.bits(d.m["p7"]))
    # all-zero gradients: no NaN; the moments decay, and the weights move by the decayed first moment only
    zeros = [[np.zeros_like(w) for w in ws]]
    opt, ps, _ = A.run_steps("cpu", ws, big[:1], **A.HYPER)
    m0 ={n: t.clone() for n, t in opt.m.items()}
    info = opt.step(A.grads_on(zeros[0]))
    assert info[0] == 0 and all(torch.isfinite(t).all() for t in ps.values())
    assert all(torch.equal(opt.m[n], torch.tensor(np.float32(0.9)) * m0[n]) for n in m0)
    ref, _ = _ref_steps(ws, big[:1] + zeros, **A.HYPER)
    assert all(np.array_equal(A.bits(ps[f"p{i}"]), A.bits(ref.w[i])) for i in range(len(ws)))
    # from a fresh optimizer zero gradients leave the weights as they are
    opt, ps, info = A.run_steps("cpu", ws, zeros, **A.HYPER)
    assert info[0, 0] == 0 and all(np.array_equal(A.bits(ps[f"p{i}"]), A.bits(ws[i])) for i in range(len(ws)))
    assert all(not t.any() for t in opt.m.values()) and all(not t.any() for t in opt.v.values())


def test_adam_annealing():
    lengths = (5, 1025)
    ws, gs = A.tensors(lengths), A.gradients(lengths, steps=9)
    hyper = dict(A.HYPER, anneal=(2, 3))  # iterations of 2 steps: lr0 x (1, 1, 2/3, 2/3, 1/3, 1/3, 0, 0, 0)
    ref, nl = _ref_steps(ws, gs, **hyper)
    opt, ps, info = A.run_steps("cpu", ws, gs, **hyper)
    A.assert_equals_ref(opt, ps, info, ref, nl, "anneal")
    lr0 = float(np.float32(2.5e-4))
    want = [np.float32(lr0 * f) for f in (1.0, 1.0, 1 - 1 / 3, 1 - 1 / 3, 1 - 2 / 3, 1 - 2 / 3, 0.0, 0.0, 0.0)]
    assert np.array_equal(A.bits(info[:, 1]), A.bits(np.array(want, np.float32)))
    # at and past the last iteration the learning rate is exactly 0 and the weights stand still
    opt6, ps6, _ = A.run_steps("cpu", ws, gs[:6], **hyper)
    assert all(np.array_equal(A.bits(ps[n]), A.bits(ps6[n])) for n in ps)
    assert not np.array_equal(A.bits(opt.m["p1"]), A.bits(opt6.m["p1"]))  # the moments still move


def test_adam_against_optax_in_float64():
    """Within 4 x the error plain torch float32 makes on the same ten steps (the convention of tests/test_gpu_ppo.py),
    at least _ppo_ref.FLOOR; both errors are measured here and printed. Observed: 1.14e-6 against torch's 2.23e-7, a
    ratio of 5.1 that only the floor of 64 * 2^-24 = 3.8e-6 admits: gca.h's running float32 products lose about
    2^-24 / (1 - b2^t) in vhat during the first steps, which `1 - b2 ** t` in double does not."""
    ws, gs = A.tensors(), A.gradients()
    gold = A.OptaxRef(ws, **A.HYPER)
    for g in gs:
        gold.step(g)
    _, ps, _ = A.run_steps("cpu", ws, gs, **A.HYPER)
    t32 = A.torch_f32_adam(ws, gs)
    err = lambda got: max(float(np.abs(np.asarray(got[i], np.float64) - gold.w[i]).max() / np.abs(gold.w[i]).max())
                          for i in range(len(ws)))
    e, e32 = err([ps[f"p{i}"].numpy() for i in range(len(ws))]), err(t32)
    print(f"adam vs optax-f64: err {e:.3e} torch-f32 {e32:.3e} ratio {e / max(e32, 1e-300):.2f}")
    assert e <= max(R.MARGIN * e32, R.FLOOR)
    moved = max(float(np.abs(gold.w[i] - ws[i]).max()) for i in range(len(ws)))
    assert moved > 1e-3  # ten steps of 2.5e-4: the comparison is not of untouched weights


def test_adam_state_dict_resumes_with_equal_bits():
    ws, gs = A.tensors(), A.gradients()
    full, pf, _ = A.run_steps("cpu", ws, gs, **A.HYPER)
    half, ph, _ = A.run_steps("cpu", ws, gs[:5], **A.HYPER)
    sd = half.state_dict()
    w5 = [ph[f"p{i}"].numpy().copy() for i in range(len(ws))]
    half.step(A.grads_on(gs[5]))  # the copies are detached from the live state
    assert int(sd["state"][0]) == 5 and A.opt_state(half)[0] == 6
    fresh, pn = A.make_opt(w5, **A.HYPER)
    fresh.load_state_dict(sd)
    for g in gs[5:]:
        fresh.step(A.grads_on(g))
    assert A.opt_state(fresh)[:3] == A.opt_state(full)[:3]
    for n in pf:
        assert np.array_equal(A.bits(pf[n]), A.bits(pn[n])) and np.array_equal(A.bits(full.v[n]), A.bits(fresh.v[n]))


def test_adam_python_errors():
    import torch

    from gymca_amd.forest_fire import ppo

    t = lambda n=4, dtype=torch.float32: torch.zeros(n, dtype=dtype)
    with pytest.raises(ValueError, match="1 to 8 tensors"):
        ppo.Adam({f"p{i}": t() for i in range(9)})
    with pytest.raises(ValueError, match="1 to 8 tensors"):
        ppo.Adam({})
    with pytest.raises(ValueError, match=r"params\['b'\]"):
        ppo.Adam({"a": t(), "b": t(dtype=torch.float64)})
    with pytest.raises(ValueError, match=r"params\['a'\]"):
        ppo.Adam({"a": torch.zeros(4, 4)[:, 1]})
    with pytest.raises(ValueError, match="anneal"):
        ppo.Adam({"a": t()}, anneal=(0, 3))
    opt = ppo.Adam({"a": t(), "b": t(3)})
    with pytest.raises(ValueError, match="names"):
        opt.step({"a": t()})
    with pytest.raises(ValueError, match=r"grads\['b'\]"):
        opt.step({"a": t(), "b": t(4)})
    with pytest.raises(ValueError, match="info_out"):
        opt.step({"a": t(), "b": t(3)}, info_out=torch.zeros(3))
    assert int(opt.count) == 0  # nothing ran


# ------------------------------------------------------------------ the permutation
def test_permutation_every_small_T():
    from gymca_amd.forest_fire import ppo

    longest = 0
    for T in A.PERM_SIZES:
        # the host build returns an error when a walk reaches the cap: a call that returns has not reached it
        got = ppo.permutation(T, 3, seed=7, epoch0=2, device="cpu").numpy()
        assert got.dtype == np.int32 and got.shape == (3, T)
        assert (np.sort(got, axis=1) == np.arange(T)).all(), T
        if T >= 8:
            assert not any(np.array_equal(got[i], got[j]) for i, j in ((0, 1), (0, 2), (1, 2))), T
        want, walks = A.permutation_ref(T, 3, 7, epoch0=2)
        longest = max(longest, walks)
        assert np.array_equal(got, want), T
    assert longest <= 64, longest  # far below the cap of 1024
    assert not np.array_equal(ppo.permutation(1000, 1, seed=8, epoch0=2, device="cpu").numpy()[0], got[0][:1000])


def test_permutation_counter_shifts_the_rows_like_epoch0():
    import torch

    from gymca_amd.forest_fire import ppo

    T = 333
    base = ppo.permutation(T, 6, seed=3, epoch0=10, device="cpu")
    counter = torch.tensor([2, 99], dtype=torch.int32)
    out = torch.full((3, T), -1, dtype=torch.int32)
    got = ppo.permutation(T, 3, seed=3, epoch0=9, counter=counter, out=out)
    assert got is out and torch.equal(out, base[1:4])
    assert torch.equal(ppo.permutation(T, 2, seed=3, epoch0=2 ** 32 - 1, counter=counter[:1]),
                       ppo.permutation(T, 2, seed=3, epoch0=1, device="cpu"))  # the key wraps modulo 2^32
    want, _ = A.permutation_ref(T, 3, 3, epoch0=9, counter=2)
    assert np.array_equal(out.numpy(), want)
    with pytest.raises(ValueError, match="out"):
        ppo.permutation(T, 3, seed=3, out=torch.zeros((3, T + 1), dtype=torch.int32))
    with pytest.raises(ValueError, match="counter"):
        ppo.permutation(T, 3, seed=3, counter=torch.zeros(1, dtype=torch.int64), out=out)


# ------------------------------------------------------------------ argument errors, both builds
def _caller(build):
    from gymca_amd import _lib

    lib = _lib.load_cpu() if build == "host" else _lib.load()

    def call(name, *args):
        return getattr(lib, name)(*args), lib.gca_last_error().decode()

    return call, lib


@pytest.mark.parametrize("build", ["host", "device"])
def test_argument_errors_and_their_messages(build):
    call, lib = _caller(build)

    def refused(text, **over):
        status, msg = A.raw_call(call, **over)
        assert status == 1 and msg == f"argument: adam: {text}", (over, status, msg)

    for over in (dict(t=None), dict(state=None), dict(ws=None), dict(t=None, n=0)):
        refused("null tensor table, state or workspace", **over)
    for n in (0, -1, 9):
        refused("1 to 8 tensors", n=n)
    for k in "wgmv":
        refused("null tensor pointer", **{k + "0": None})
    refused("tensor lengths in [1, 2^31)", len0=0)
    refused("tensor lengths in [1, 2^31)", len0=2 ** 31, b1=1.0)
    for over in (dict(w0=0x10002), dict(v0=0x10301), dict(state=0x20002), dict(info=0x40001)):
        refused("tensors, state and info_out 4-B aligned", **over)
    refused("workspace 8-B aligned", ws=0x30004)
    for over in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan")), dict(b1=1.0, eps=-1.0)):
        refused("b1 and b2 in [0, 1)", **over)
    refused("eps >= 0", eps=-1e-8)
    for spi, ni in ((1, 0), (0, 1), (-1, -1), (2, -3)):
        refused("steps_per_iteration and num_iterations both 0 (no annealing) or both >= 1", spi=spi, ni=ni)
    refused("workspace smaller than gca_adam_step_workspace", ws_bytes=63)
    refused("workspace smaller than gca_adam_step_workspace", ws_bytes=0)
    # the workspace query: 8 bytes per chunk of the concatenated tensors plus one tail per tensor
    assert lib.gca_adam_step_workspace(1) == 64 and lib.gca_adam_step_workspace(70001 + 3077) == 8 * (71 + 8)
    assert lib.gca_adam_step_workspace(2 ** 22) == 8 * (2048 + 8)  # chunks of 2048 elements
    assert lib.gca_adam_step_workspace(0) == -1
    assert lib.gca_last_error().decode() == "argument: adam_step_workspace: total_elements >= 1"

    def perm_refused(text, seed=1, epoch0=0, counter=None, T=10, rows=2, out=0x50000):
        status, msg = call("gca_permutation", seed, epoch0, counter, T, rows, out, None)
        assert status == 1 and msg == f"argument: permutation: {text}", (status, msg)

    perm_refused("null out", out=None)
    perm_refused("null out", out=None, T=0)
    perm_refused("1 <= T < 2^31", T=0)
    perm_refused("1 <= T < 2^31", T=2 ** 31, rows=0)
    perm_refused("1 <= rows <= 65535", rows=0)
    perm_refused("1 <= rows <= 65535", rows=65536)
    perm_refused("out and counter 4-B aligned", out=0x50002)
    perm_refused("out and counter 4-B aligned", counter=0x60001)


def test_adam_tensors_layout_matches_the_header(tmp_path):
    import os
    import subprocess

    from conftest import ROOT
    from gymca_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gca.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %d %d %u\\n", sizeof(gca_adam_tensors), offsetof(gca_adam_tensors, len),'
                   ' offsetof(gca_adam_tensors, w), offsetof(gca_adam_tensors, g), offsetof(gca_adam_tensors, m),'
                   ' offsetof(gca_adam_tensors, v), GCA_ADAM_MAX_TENSORS, GCA_ADAM_STATE_WORDS, GCA_TAG_PERM);\n'
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = _lib.AdamTensors
    assert got == [ctypes.sizeof(T), T.len.offset, T.w.offset, T.g.offset, T.m.offset, T.v.offset,
                   _lib.GCA_ADAM_MAX_TENSORS, _lib.GCA_ADAM_STATE_WORDS, _lib.TAG_PERM]
