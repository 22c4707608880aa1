"""CPU: bench.py's roofline provenance — traffic / valu_busy come from the committed profile of the timed kernel
(template instance AND source hash), never from another build's entry (VERDICT r03 "what's weak" 4)."""
import json
import os
import shutil
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def _tree(tmp_path):
    for d in ("gym-cellular-automata_amd/csrc", "include", "profiles"):
        (tmp_path / d).mkdir(parents=True)
    for f in ("gca_alex_march.hip", "gca_alex_rule.h", "gca_common.h", "gca_alex.hip"):
        shutil.copy(os.path.join(ROOT, "gym-cellular-automata_amd", "csrc", f), tmp_path / "gym-cellular-automata_amd/csrc" / f)
    shutil.copy(os.path.join(ROOT, "include", "gca.h"), tmp_path / "include" / "gca.h")


def test_headline_key_names_the_launched_template():
    bench = _bench()
    p = types.SimpleNamespace(R=6, p_tree=0.0)
    env = types.SimpleNamespace(alex_params=p, march=True, slope_layout="packed", ncols=256)
    assert bench.headline_kernel_key(env) == "alex_march<6, false, false, 1, 0>"
    p.p_tree = 0.5
    assert bench.headline_kernel_key(env) == "alex_march<6, false, true, 1, 0>"
    env.ncols = 512
    assert bench.headline_kernel_key(env) == "alex_march<6, false, true, 2, 0>"
    env.flat_terrain = True  # edge_slope = NULL: the flat-terrain instance
    assert bench.headline_kernel_key(env) == "alex_march<6, false, true, 2, 1>"
    env.uniform_layers = True  # vd = NULL too
    assert bench.headline_kernel_key(env) == "alex_march<6, false, true, 2, 2>"
    env = types.SimpleNamespace(alex_params=types.SimpleNamespace(R=7, p_tree=0.0), march=False, slope_layout="packed")
    assert bench.headline_kernel_key(env) == "alex_step<7, 0, true, true, true, false>"
    env.slope_layout = "planes"
    assert bench.headline_kernel_key(env) == "alex_step<7, 0, true, false, false, false>"


def test_profile_entry_requires_the_same_sources(tmp_path, monkeypatch):
    bench = _bench()
    _tree(tmp_path)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    key = "alex_march<6, false, false, 1>"
    sha = bench.kernel_src_sha(key)
    assert sha and sha == bench.kernel_src_sha("alex_march<6, false, true, 2>")  # one family, one source set
    args = types.SimpleNamespace(envs=4096, size=256)
    entry = {"bytes_per_launch": 7.0e9, "valu_busy": 0.9, "tag": "rX", "src_sha": sha}
    (tmp_path / "profiles" / "pmc_traffic.json").write_text(json.dumps({key: entry, "alex_march<6, false>": {
        "bytes_per_launch": 1.0, "tag": "old"}}))
    e, info = bench.profile_entry(args, key)
    assert e["bytes_per_launch"] == 7.0e9 and info["match"] and info["tag"] == "rX"
    # another template instance of the same family: no entry -> null, never a neighbour's figures
    e, info = bench.profile_entry(args, "alex_march<6, true, false, 1>")
    assert e is None and not info["match"]
    # an entry without a source stamp (older profile) -> null
    e, info = bench.profile_entry(args, "alex_march<6, false>")
    assert e is None and "predates" in info["why"]
    # the kernel's source changes after profiling -> null
    with open(tmp_path / "gym-cellular-automata_amd/csrc/gca_alex_march.hip", "a") as f:
        f.write("\n// changed\n")
    e, info = bench.profile_entry(args, key)
    assert e is None and info["profile_src_sha"] == sha and info["src_sha"] != sha
    # not the profiled workload -> null
    e, info = bench.profile_entry(types.SimpleNamespace(envs=1024, size=256), key)
    assert e is None


def test_plain_run_is_the_headline_loop_alone(monkeypatch):
    """Without --full: one repetition of exactly --steps steps, no CPU legs, no secondary sections; --full restores
    the 5 repetitions and every section."""
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.reps) == (7, 2, 1) and not a.full and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_secondary
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.reps == 5 and a.dump_outputs == "d" and not a.no_cpu_baseline and not a.no_secondary


def test_dump_outputs_writes_float32_arrays_of_a_fixed_env_sample(tmp_path):
    """--dump-outputs: grid / fire age of the same seeded env sample on every call, the per-env results of every env,
    all float32 .npy files."""
    import numpy as np
    import torch

    bench = _bench()
    E = 3 * bench.DUMP_ENVS
    grid = torch.arange(2 * E * 4 * 4, dtype=torch.int64).reshape(2, E, 4, 4).remainder(3).to(torch.uint8)
    age = torch.arange(2 * E * 4 * 4, dtype=torch.int64).reshape(2, E, 4, 4).remainder(673).to(torch.int16)
    per_env = {k: torch.arange(E, dtype=dt) for k, dt in (
        ("reward", torch.float32), ("done", torch.uint8), ("steps_elapsed", torch.float32),
        ("reward_accumulated", torch.float32), ("wind_index", torch.int32), ("time_step", torch.int32))}
    env = types.SimpleNamespace(num_envs=E, cur=1, grid=grid, age=age, counts=torch.ones((E, 3), dtype=torch.int32),
                                pos=torch.zeros((E, 2), dtype=torch.int32), **per_env)
    out = bench.headline_outputs(env)
    idx = out["env_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_ENVS == len(set(idx.tolist())) and np.array_equal(idx, np.sort(idx))
    assert np.array_equal(bench.headline_outputs(env)["env_index"], out["env_index"])
    assert np.array_equal(out["grid"], grid[1].numpy()[idx]) and np.array_equal(out["fire_age"], age[1].numpy()[idx])
    assert out["reward"].shape == (E,) and out["counts"].shape == (E, 3)
    bench.write_outputs(str(tmp_path / "d"), out)
    for name, a in out.items():
        b = np.load(tmp_path / "d" / f"{name}.npy")
        assert b.dtype == np.float32 and np.array_equal(a, b), name


def test_algorithmic_bytes_follow_the_launched_instance():
    """roofline.algorithmic_bytes_per_cell is that of the step the env launches: the packed layout's 23.125 B, minus the
    16 B of slope planes on flat terrain, minus the layer byte with uniform layers (tiled / other layouts unchanged)."""
    bench = _bench()
    env = types.SimpleNamespace(march=True, flat_terrain=False, uniform_layers=False)
    assert bench.alex_bytes(env, "packed") == 23.125
    env.flat_terrain = True
    assert bench.alex_bytes(env, "packed") == 7.125
    env.uniform_layers = True
    assert bench.alex_bytes(env, "packed") == 6.125
    env.march = False  # the tiled step reads every plane
    assert bench.alex_bytes(env, "packed") == 23.125
    assert bench.alex_bytes(types.SimpleNamespace(), "planes") == 41
