"""host logic of bench.py that needs no GPU: which committed counter profile a run may quote for roofline.traffic, the
outputs --dump-outputs writes, the argument checks"""
import json
import os
import sys

from conftest import REPO

sys.path.insert(0, REPO)


class _Lib:
    def __init__(self, hashes):
        self.h = hashes

    def snk_source_hash(self, name):
        v = self.h.get(name.decode())
        return None if v is None else v.encode()


def test_traffic_profile_is_quoted_only_for_the_sources_and_form_it_was_measured_on(tmp_path):
    import bench
    have = {"conv_split.hip": "a" * 64, "common.h": "b" * 64}
    prof = {"conv_algo": "f16s", "rect_layers": 6, "source_sha256": dict(have), "hbm_bytes_per_state_layer": 400000.0}
    json.dump(prof, open(tmp_path / "rX_conv_traffic.json", "w"))
    json.dump({"hbm_bytes_per_state_layer": 1.0}, open(tmp_path / "old_traffic.json", "w"))      # a profile without provenance
    per_launch = 2.0 * 441 * 9 * 128 * 128 * 1000                                               # a launch of 1 000 states
    t, src = bench.conv_traffic_profile(_Lib(have), "f16s", 6, per_launch, str(tmp_path))
    assert t == 400000.0 * 1000 and src.endswith("rX_conv_traffic.json")
    for lib_, algo, n_rect in ((_Lib(dict(have, **{"conv_split.hip": "c" * 64})), "f16s", 6),     # the kernel source changed
                               (_Lib(have), "f16a", 6), (_Lib(have), "f16s", 0), (_Lib({}), "f16s", 6)):
        t, why = bench.conv_traffic_profile(lib_, algo, n_rect, per_launch, str(tmp_path))
        assert t is None and "no profile" in why


def test_committed_traffic_profiles_with_provenance_are_well_formed():
    import glob
    for path in glob.glob(os.path.join(REPO, "profiles", "*traffic.json")):
        d = json.load(open(path))
        if "source_sha256" in d:
            assert set(d["source_sha256"]) == {"conv_split.hip", "common.h"} and all(len(v) == 64 for v in d["source_sha256"].values())
            assert d["conv_algo"] in ("f16s", "f16a", "bf16", "f16") and d["kernel_symbols"] and d["hbm_bytes_per_state_layer"] > 0


def test_counter_profile_is_quoted_only_for_the_sources_tower_and_board_it_was_taken_on(tmp_path):
    """round 6: roofline.counters / counters_source follow the rule of traffic / traffic_source -- SQ counters of
    another build of csrc/conv_split.hip, another tower or another canvas are not this run's counters"""
    import bench
    have = {"conv_split.hip": "a" * 64, "common.h": "b" * 64}
    kern = {"k_conv3x3_f16s<7, 1, true, 0, false>": {"dispatches": 4, "per_dispatch": {"SQ_INSTS_MFMA": 8.0e7},
                                                     "derived": {"mfma_busy_per_busy_cycle": 25.6, "lds_conflict_share": 0.46,
                                                                 "sq_wait_inst_any_share_of_wave_cycles": 0.58, "valu_instructions_per_mfma": 3.0}},
            "k_f16s_wscale": {"dispatches": 1, "per_dispatch": {"SQ_INSTS_MFMA": 0.0}, "derived": {}}}
    prof = {"source_sha256": dict(have, **{"engine.hip": "e" * 64}), "kernels": kern,
            "note": "tools/pmc_tower.sh r6_f16s f16s 2300 11: tools/tower_only.py 2300 2 11 with SNK_CONV_ALGO=f16s (two forwards ...)"}
    json.dump(prof, open(tmp_path / "rX_conv_f16s_sq_counters.json", "w"))
    c, src = bench.conv_counters_profile(_Lib(have), "f16s", 11, str(tmp_path))
    assert src.endswith("rX_conv_f16s_sq_counters.json") and list(c) == ["k_conv3x3_f16s<7, 1, true, 0, false>"]
    row = c["k_conv3x3_f16s<7, 1, true, 0, false>"]
    assert abs(row["mfma_busy_share"] - 0.8) < 1e-12 and row["lds_conflict_share"] == 0.46 and row["valu_per_mfma"] == 3.0
    for lib_, algo, board in ((_Lib(dict(have, **{"conv_split.hip": "c" * 64})), "f16s", 11), (_Lib(have), "bf16", 11),
                              (_Lib(have), "f16s", 19), (_Lib({}), "f16s", 11)):
        c, why = bench.conv_counters_profile(lib_, algo, board, str(tmp_path))
        assert c is None and "no SQ-counter profile" in why
    # round 5's file (pmc_a16.sh's note: "... tower_only.py 500 2 19 with SNK_CONV_ALGO=bf16 ...") is found for the bf16 tower at 19
    prof19 = dict(prof, note="tools/pmc_a16.sh r5_bf16: tools/tower_only.py 500 2 19 with SNK_CONV_ALGO=bf16 (two forwards ...)",
                  kernels={"k_conv3x3_f16s<8, 1, false, 3, true>": kern["k_conv3x3_f16s<7, 1, true, 0, false>"]})
    json.dump(prof19, open(tmp_path / "rY_a16_sq_counters.json", "w"))
    c, src = bench.conv_counters_profile(_Lib(have), "bf16", 19, str(tmp_path))
    assert src.endswith("rY_a16_sq_counters.json") and list(c) == ["k_conv3x3_f16s<8, 1, false, 3, true>"]


def test_dumped_outputs_are_the_last_steps_arrays_in_float32(tmp_path):
    """--dump-outputs: the moves, root values and rewards land at their [game, snake], all finite, the board of every game after the step, a
    fixed sample of the step's observations and of the exchange rows; the same inputs give the same files"""
    import numpy as np
    import torch
    import bench
    from snake_engine._lib import SnkGameState
    G, S, OBS = 10, 4, 21

    class Eng:
        def export(self, slots=None):
            arr = (SnkGameState * len(slots))()
            for i, s in enumerate(slots):
                arr[i].H = arr[i].W = 11
                arr[i].S = S
                arr[i].health[0] = int(s)
            return arr

    class Runner:
        game_cnt, snake_cnt, engine = G, S, Eng()

    class Records:
        def __len__(self):
            return 30

        def fetch_device(self, idx):           # record i's observation is filled with i
            return torch.as_tensor(np.asarray(idx, np.float32))[:, None, None, None].expand(-1, OBS, OBS, 3)

    class Agent:
        records = Records()
        _rec_values = [np.zeros((1, 3), np.float32), np.arange(36, dtype=np.float32).reshape(12, 3)]
    ids = [(g, s) for g in range(3, 9) for s in (0, 2)]
    rewards = [None] * G
    rewards[1] = [1.0, None, -1.0, None]
    Xg, Vg = torch.rand(50, OBS, OBS, 3), torch.rand(50, 3)
    out = bench.last_step_outputs(Runner(), Agent(), ids, [1, 2] * 6, rewards, Xg, Vg, max_obs=8)
    assert all(v.dtype == np.float32 for v in out.values())
    assert all(np.isfinite(v).all() for v in out.values())
    assert out["asked"].sum() == 12 and out["asked"][3].tolist() == [1, 0, 1, 0] and not out["asked"][0].any()
    assert out["moves"][3].tolist() == [1, -1, 2, -1] and (out["moves"][0] == -1).all()
    assert out["root_values"][8, 2].tolist() == [33, 34, 35] and not out["root_values"][0].any()
    assert out["rewards"][1].tolist() == [1.0, 0.0, -1.0, 0.0] and not out["rewards"][0].any()
    assert out["state_health"][:, 0].tolist() == list(range(G)) and out["state_food"].shape == (G, 121)
    assert out["observations"].shape == (8, OBS, OBS, 3) and out["observations"][:, 0, 0, 0].min() >= 30 - 12
    rec = out["observations"][:, 0, 0, 0].astype(int) - 18                    # which of the step's 12 records were sampled
    assert out["observation_ids"].tolist() == [list(ids[i]) for i in rec]
    assert np.array_equal(Xg[out["exchange_rows"].astype(np.int64)].numpy(), out["exchange_observations"]) and len(out["exchange_rows"]) == 8
    again = bench.last_step_outputs(Runner(), Agent(), ids, [1, 2] * 6, rewards, Xg, Vg, max_obs=8)
    assert all(np.array_equal(out[k], again[k]) for k in out)
    bench.write_outputs(str(tmp_path / "o"), out)
    assert sorted(os.listdir(tmp_path / "o")) == sorted(k + ".npy" for k in out)
    import pytest
    with pytest.raises(RuntimeError, match="more than"):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros((17 << 20,), np.float32)})
    with pytest.raises(RuntimeError, match="non-finite values in x"):
        bench.write_outputs(str(tmp_path / "nan"), {"x": np.array([0.0, np.nan], np.float32)})


def test_steps_must_be_positive():
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--steps" in out.stderr
