"""The rules both engine wrappers and both vector adapters share (engine_handle.py, host_mirror.py), checked without a
GPU and, but for the last test, without the native library: seeds, PCG64 words, grids, the layout of the blob of small
outputs, and the host mirror's view arithmetic.  The expected values are those the wrappers' own constructors computed
before the rules were gathered in one place."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dl_reference_models_amd import engine_handle as eh
from dl_reference_models_amd import evaluation, vec_env, vec_env_single_agent
from dl_reference_models_amd.host_mirror import HostMirror

WORDS = np.arange(18, dtype=np.uint64).reshape(3, 6)


def test_config_seeds():
    assert eh.config_seeds({"seed": 7}, 3) == [7, 8, 9]
    assert eh.config_seeds({}, 3) == [None] * 3
    assert eh.config_seeds({"seed": None, "seeds": None}, 3) == [None] * 3
    assert eh.config_seeds({"seeds": [5, None, 11], "seed": 7}, 3) == [5, None, 11]  # explicit seeds win over seed
    assert eh.config_seeds({"seeds": np.array([4, 2, 9])}, 3) == [4, 2, 9]
    for bad in ([1, 2], [1, 2, 3, 4], []):
        with pytest.raises(ValueError, match="need one seed per env"):
            eh.config_seeds({"seeds": bad}, 3)
    # rng_words replaces the streams, not the seed list: it is config_rng_words that lets it override
    assert eh.config_seeds({"seed": 7, "rng_words": WORDS}, 3) == [7, 8, 9]


@pytest.mark.parametrize("cfg", [{"seed": 7}, {}, {"seeds": [5, None, 11]}, {"seeds": np.array([4, 2, 9]), "seed": 1},
                                 {"rng_words": WORDS}, {"rng_words": WORDS, "seed": 7}, {"rng_words": WORDS, "seeds": [1, 2, 3]}])
def test_evaluation_env_seeds_agrees_with_config_seeds(cfg):
    got = evaluation.env_seeds(SimpleNamespace(env_config=cfg, num_envs=3))
    if "rng_words" in cfg:
        assert got == [None] * 3
    else:
        assert got == eh.config_seeds(cfg, 3)
        assert all(s is None or type(s) is int for s in got)


def test_config_rng_words():
    for s in (0, 7, 2**40):
        assert np.array_equal(eh.config_rng_words({"seed": s}, 3), np.stack([eh.pcg64_words(s + b) for b in range(3)]))
    assert np.array_equal(eh.config_rng_words({"seeds": [9, 1]}, 2), np.stack([eh.pcg64_words(9), eh.pcg64_words(1)]))
    w = eh.config_rng_words({"seed": 7}, 3)
    assert w.dtype == np.uint64 and w.shape == (3, 6) and w.flags.c_contiguous
    # the words are the generator's state: a stream rebuilt from them draws what default_rng(seed) draws
    st = np.random.PCG64().state
    st["state"] = {"state": (int(w[1, 0]) << 64) | int(w[1, 1]), "inc": (int(w[1, 2]) << 64) | int(w[1, 3])}
    st["has_uint32"], st["uinteger"] = int(w[1, 4]), int(w[1, 5])
    bg = np.random.PCG64()
    bg.state = st
    assert np.array_equal(np.random.Generator(bg).integers(0, 1000, 8), np.random.default_rng(8).integers(0, 1000, 8))
    # explicit words override seeds, whatever those are, and come back as uint64 [B,6]
    got = eh.config_rng_words({"rng_words": WORDS.reshape(-1).tolist(), "seed": 7, "seeds": [1]}, 3)
    assert got.dtype == np.uint64 and np.array_equal(got, WORDS)
    with pytest.raises(ValueError, match="need one seed per env"):
        eh.config_rng_words({"seeds": [1, 2]}, 3)
    assert vec_env.pcg64_words is eh.pcg64_words  # (the name bench.py, the oracle and the tests import)


def test_config_grids():
    g2 = np.array([[0, 1, 0], [0, 0, 0]])
    grids, shared = eh.config_grids({"grid": g2}, 4)
    assert shared == 1 and grids.shape == (1, 2, 3) and grids.dtype == np.uint8 and np.array_equal(grids[0], g2)
    g3 = np.stack([g2] * 4)
    grids, shared = eh.config_grids({"grid": g3.tolist()}, 4)
    assert shared == 0 and grids.shape == (4, 2, 3) and grids.dtype == np.uint8 and grids.flags.c_contiguous
    for bad in (np.stack([g2] * 5), np.stack([g2] * 3), np.zeros(6), np.zeros((1, 1, 2, 3))):
        with pytest.raises(ValueError, match=r"grid must be \[H,W\] or \[num_envs,H,W\]"):
            eh.config_grids({"grid": bad}, 4)
    from dl_reference_models_amd import get_grid as gg

    grids, shared = eh.config_grids({"env_name": "ReferenceModel-2-1"}, 2)
    assert shared == 1 and np.array_equal(grids[0], np.asarray(gg.get_grid("ReferenceModel-2-1"), dtype=np.uint8))


def test_config_fixed_tables():
    fs, fg = eh.config_fixed_tables({"fixed_starts": [[0, 0], [1, 2]], "fixed_goals": [[1, 2], [0, 0]]}, 2, 3)
    assert fs.shape == fg.shape == (3, 2, 2) and fs.dtype == fg.dtype == np.int16 and fs.flags.c_contiguous
    assert np.array_equal(fs, np.broadcast_to([[0, 0], [1, 2]], (3, 2, 2))) and np.array_equal(fg[2], [[1, 2], [0, 0]])
    per_env = np.arange(12).reshape(3, 2, 2)
    fs, _ = eh.config_fixed_tables({"fixed_starts": per_env, "fixed_goals": per_env}, 2, 3)
    assert np.array_equal(fs, per_env)
    from dl_reference_models_amd import get_grid as gg

    # one table alone counts as neither: both come from the named grid
    fs, fg = eh.config_fixed_tables({"env_name": "ReferenceModel-2-1", "fixed_starts": [[0, 0], [1, 2]]}, 2, 2)
    s, g = gg.get_start_positions("ReferenceModel-2-1", 2), gg.get_goal_positions("ReferenceModel-2-1", 2)
    assert np.array_equal(fs[1], [s["agent_0"], s["agent_1"]]) and np.array_equal(fg[0], [g["agent_0"], g["agent_1"]])


# offsets and total of _out_blob as the constructors' own packing loop gave them, worked out by hand: section sizes in
# bytes are (B*N*4, B*14*4, B*N*2, B, B) for the multi-agent env and (B*8, B*4*4, B, B) for the single-agent one
KNOWN_LAYOUTS = [
    (vec_env.output_sections(3, 2), [24, 168, 12, 3, 3], [0, 256, 512, 768, 1024], 1280),
    (vec_env.output_sections(64, 4), [1024, 3584, 512, 64, 64], [0, 1024, 4608, 5120, 5376], 5632),
    (vec_env_single_agent.output_sections(3), [24, 48, 3, 3], [0, 256, 512, 768], 1024),
]


@pytest.mark.parametrize("sections,sizes,offsets,total", KNOWN_LAYOUTS)
def test_section_layout(sections, sizes, offsets, total):
    offs, szs, tot = eh.section_layout(sections)
    assert (offs, szs, tot) == (offsets, sizes, total)
    assert all(o % 256 == 0 for o in offs)
    assert all(o + s <= nxt for o, s, nxt in zip(offs, szs, offs[1:] + [tot]))  # no overlap, nothing past the end
    assert tot == sum((s + 255) // 256 * 256 for s in szs)


def test_section_names_are_the_attributes_the_wrappers_expose():
    assert [n for n, _, _ in vec_env.output_sections(1, 1)] == ["_rewards", "_info_all", "_info_agent", "_terminated",
                                                                "_truncated"]
    assert [n for n, _, _ in vec_env_single_agent.output_sections(1)] == ["_reward", "_info", "_terminated", "_truncated"]


@pytest.mark.parametrize("sections,np_dtypes", [
    (vec_env.output_sections(3, 2), (np.float32, np.float32, np.uint8, np.uint8, np.uint8)),
    (vec_env_single_agent.output_sections(3), (np.float64, np.float32, np.uint8, np.uint8)),
])
def test_host_mirror_views_show_the_sections_of_the_copied_blob(sections, np_dtypes):
    blob, views = eh.alloc_sections(sections, "cpu")  # a CPU stand-in for the engine's device blob
    assert blob.dtype == torch.uint8 and blob.numel() == eh.section_layout(sections)[2] and not blob.any()
    eng = SimpleNamespace(_obs=torch.zeros((3, 5)), _out_blob=blob, **views)
    m = HostMirror(eng)
    assert tuple(m._h_obs.shape) == (3, 5) and m._h_blob.shape == blob.shape
    m._h_blob.zero_()
    host = {name: m.view(views[name], dt) for (name, _, _), dt in zip(sections, np_dtypes)}
    want = {}
    for k, (name, shape, _) in enumerate(sections):  # write through the "device" views, a different pattern per section
        want[name] = (np.arange(int(np.prod(shape))).reshape(shape) % 7 + k + 1).astype(host[name].dtype)
        views[name].copy_(torch.from_numpy(want[name]))
    assert not any(v.any() for v in host.values())  # nothing shows before the copy
    m._h_blob.copy_(blob)
    for (name, shape, _), dt in zip(sections, np_dtypes):
        assert host[name].dtype == dt and host[name].shape == shape
        assert np.array_equal(host[name], want[name]), name
    # the views alias the mirror (no copy per step), and together they cover exactly the sections' bytes
    assert all(np.shares_memory(v, m._h_blob.numpy()) for v in host.values())
    assert int((m._h_blob != 0).sum()) <= sum(eh.section_layout(sections)[1])


@pytest.mark.parametrize("module,cls", [("vec_env", "VecReferenceModel"),
                                        ("vec_env_single_agent", "VecSingleAgentReferenceModel")])
def test_both_wrappers_refuse_a_cpu_device_and_a_grid_stack_of_the_wrong_length(module, cls):
    # (this one loads the native library, as the constructors do first; nothing reaches a device)
    import importlib

    model = getattr(importlib.import_module("dl_reference_models_amd." + module), cls)
    grid = np.zeros((4, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match=cls + " runs on a HIP device only"):
        model({"grid": grid, "device": "cpu"})
    with pytest.raises(ValueError, match=r"grid must be \[H,W\] or \[num_envs,H,W\]"):
        model({"grid": np.stack([grid] * 3), "num_envs": 2, "device": "cuda:0"})
