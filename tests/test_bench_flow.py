"""bench.py's contract, exercised end to end on CPU (kernel emulator): one JSON line from rank 0 with the required
fields, for N = 1 and for N = 2 launched exactly like the driver launches it (torch.distributed.run, one process per
rank) -- in particular the roofline leg, whose extra steps contain gradient all-reduces and therefore must be run
by every rank."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "tests", "bench_flow_runner.py")
ARGS = ["--steps", "2", "--warmup", "1", "--batch", "2", "--image-size", "64", "--vocab-size", "304", "--dtype", "bf16",
        "--textual", "transdec_postnorm::L1_H128_A2_F256", "--no-cpu-baseline", "--roofline-steps", "1",
        "--launch", "eager",      # (launch replay has its own tests: on the emulator its warm-up / validation / recording steps cost minutes)
        "--full"]                 # the secondary legs (roofline, fidelity, CPU baseline) run only on request
REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"}


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_single_rank_flow():
    args = [x for x in ARGS if x != "--no-cpu-baseline"] + ["--cpu-batch", "1", "--cpu-steps", "1"]   # with the CPU baseline leg
    r = subprocess.run([sys.executable, RUNNER, "--gpus", "1"] + args, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    assert REQUIRED <= set(rec) and rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["metric"] == "pretrain images/sec" and rec["value"] > 0 and rec["scaling"] == "weak"
    roof = rec["roofline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_us"} <= set(roof)
    assert isinstance(roof["kernel"], str) and roof["kernel"] and roof["launches"] > 0
    # every kernel of the step is timed, not only the contractions: HBM GB/s per norm / embedding / loss / optimizer kernel,
    # per-family sums and the step-level sum of max(t_MFMA, t_HBM)
    assert {"bn_fwd_apply", "bn_bwd_apply", "layernorm_fwd", "embedding_fwd", "optimizer_step"} <= set(roof["hbm_kernels"])
    assert all({"GB/s", "frac", "ms_per_step"} <= set(v) for v in roof["hbm_kernels"].values())
    assert {"batchnorm", "contractions (MFMA)", "layernorm", "optimizer"} <= set(roof["families"])
    assert 0 < roof["step_model"]["sum_max_mfma_hbm_ms"] and roof["step_model"]["measured_kernel_ms"] > 0
    # the headline is ONE kernel instantiation (the largest class of the fully timed step); the family-merged pick and the two
    # step-level fractions sit beside it.  (Fractions above 1 are legitimately possible HERE: the emulator's event times are
    # host times of a CPU run, so only the presence of the verdict is asserted.)
    assert {"dominant_family", "step_model_frac", "step_mfma_frac", "consistency", "selection"} <= set(roof)
    assert roof["dominant_family"]["instantiations"] >= 1 and "|" not in roof["kernel"] and "family:" not in roof["kernel"]
    fid = rec["fidelity"]
    assert "error" not in fid and fid["backbone"]["tensors"] > 0 and fid["text"]["tensors"] == 43 and fid["loss_rel"] < 1e-2
    cpu = rec["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["unit"] == "images/sec"
    assert cpu["config1_bs2"]["value"] > 0


def test_plain_run_times_the_steps_and_dumps_what_the_last_one_computed(tmp_path):
    """Without --full: set-up, warm-up, the timed steps, the line -- no secondary leg.  --dump-outputs writes the last timed
    step's loss, parameters and gradients as float32 .npy files (this toy model is small enough to be written whole)."""
    import numpy as np
    args = [x for x in ARGS if x != "--full"] + ["--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run([sys.executable, RUNNER, "--gpus", "1"] + args, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    assert (REQUIRED - {"roofline"}) <= set(rec) and rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert not {"roofline", "fidelity", "cpu_baseline", "stock_pytorch_baseline"} & set(rec)
    # batch 2: images/sec from the timed steps alone (`value` is printed with two decimals: half a unit of the last one)
    assert rec["value"] == pytest.approx(2 * 1e3 / rec["ms_per_step"], rel=1e-3, abs=0.005)
    assert sorted(os.listdir(tmp_path / "out")) == ["gradients.npy", "loss.npy", "parameters.npy"]
    out = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in ("loss", "parameters", "gradients")}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in out.values())
    assert out["loss"].shape == (1,) and float(out["loss"][0]) == pytest.approx(rec["config"]["final_loss"], abs=1e-4)
    assert out["parameters"].shape == out["gradients"].shape and out["parameters"].ndim == 1 and np.abs(out["gradients"]).max() > 0
    assert sum(v.nbytes for v in out.values()) <= 64e6


def test_two_rank_flow_does_not_deadlock_in_the_roofline_leg():
    env = dict(os.environ, OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29631", RUNNER, "--gpus", "2"] + ARGS
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rec = _json_line(r.stdout)
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 4 and rec["config"]["parallelism"] == "dp2"
    assert rec["roofline"] is not None and "cpu_baseline" not in rec and "error" not in rec["fidelity"]
    # "did the transport see N ranks" is answerable from the record; N > 1 times the eager step unless replay is opted in
    dp = rec["data_parallel"]
    assert dp["ranks_seen"] == 2 and dp["world_size"] == 2 and dp["backend"] == "gloo" and dp["launch"] == "eager"
    assert dp["buffers_broadcast_before_validation"] is True and rec["config"]["launch"] == "eager"


def test_auto_launch_is_eager_for_more_than_one_rank(monkeypatch):
    """bench.py --launch auto: replay only for the single-process run unless VIRTEX_AMD_REPLAY_DP=1 (the recorded list with
    collectives has never run on RCCL x N)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'replay_ok = world == 1 or os.environ.get("VIRTEX_AMD_REPLAY_DP", "0") == "1"' in src
    assert 'want = "replay" if (dev.type == "cuda" and not a.roofline_live and replay_ok) else "eager"' in src


def test_roofline_headline_is_the_largest_single_instantiation():
    sys.path.insert(0, ROOT)
    import bench
    recs = [
        {"cls": 0, "name": "family:bn_bwd_apply|(bn_bwd_apply_fused_kernel<T, UNR, true>)|[T = unsigned short, UNR = 2]", "launches": 47,
         "seconds": 1.7e-3, "flops": 0.0, "bytes": 47 * 2.0e8},
        {"cls": 1, "name": "family:bn_bwd_apply|(bn_bwd_apply_fused_kernel<T, UNR, true>)|[T = unsigned short, UNR = 4]", "launches": 3,
         "seconds": 0.6e-3, "flops": 0.0, "bytes": 3 * 1.2e9},
        {"cls": 2, "name": "[BM = 128, BN = 128, WM = 2, WN = 2, BK = 32, STAGES = 3, AL = vtxg::PlainKC<unsigned short, 2>, "
                           "BL = vtxg::PlainKC<unsigned short, 2>, EP = vtxg::EpiStore<unsigned short, 2>]", "launches": 19,
         "seconds": 2.0e-3, "flops": 19 * 5e9, "bytes": 19 * 5.5e8},
        {"cls": 3, "name": "family:optimizer_step|sgd_lookahead_kernel|", "launches": 1, "seconds": 0.25e-3, "flops": 0.0, "bytes": 1.39e9},
    ]
    # merged by family the BatchNorm backward applies (2.3 ms) are ahead of the join class (2.0 ms); the headline is the join class
    assert bench.dominant_class(recs)["cls"] == 2
    roof = bench.step_roofline(recs, "bf16", None)
    assert roof["kernel"].startswith("contraction_v2_kernel<128, 128, 2, 2, PlainKC<bf16, 2>") and roof["launches"] == 19
    assert roof["dominant_family"]["family"] == "bn_bwd_apply" and roof["dominant_family"]["instantiations"] == 2
    assert abs(roof["hbm_frac"] - 19 * 5.5e8 / 2.0e-3 / 8e12) < 1e-3 and roof["bound"] == "hbm"
    assert bench._instantiation_name(recs[0]["name"]) == "bn_bwd_apply_fused_kernel<bf16, 2, true>"
    assert bench._instantiation_name(recs[3]["name"]) == "sgd_lookahead_kernel" and bench._display_name(recs[3]["name"]) == "optimizer_step"
    assert bench.roofline_violations(roof) == []
    recs[3]["bytes"] = 2.5e9            # 10 TB/s: more than the part has
    bad = bench.roofline_violations(bench.step_roofline(recs, "bf16", None))
    assert bad and any("optimizer_step" in b for b in bad)


def test_single_rank_flow_through_the_data_parallel_engine():
    """VIRTEX_AMD_FORCE_DIST keeps the engine (process group, parameter broadcast, bucket all-reduces, barriers) in the
    loop with one rank -- the CPU twin of tests/test_distributed_gpu.py::test_bench_through_rccl_with_one_rank."""
    env = dict(os.environ, VIRTEX_AMD_FORCE_DIST="gloo", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29633", VIRTEX_AMD_DP_PAYLOAD="bf16")
    r = subprocess.run([sys.executable, RUNNER, "--gpus", "1"] + ARGS + ["--no-roofline"], capture_output=True, text=True,
                       timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    assert rec["n_gpus"] == 1 and rec["value"] > 0 and "error" not in rec["fidelity"]


def test_traffic_table_is_keyed_to_the_kernel_sources(tmp_path, monkeypatch, capsys):
    """roofline.traffic comes from profiles/traffic_table.json only while the sha256 of the kernel sources it was measured on
    matches the tree (virtex_amd.build.csrc_hash); a stale or missing table yields no number and an error on stderr."""
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from virtex_amd.build import csrc_hash
    p = tmp_path / "traffic_table.json"
    monkeypatch.setattr(bench, "TRAFFIC_TABLE", str(p))
    table, src = bench.load_traffic_table()
    assert table == {} and src is None and "missing" in capsys.readouterr().err
    p.write_text(json.dumps({"csrc_sha256": "0" * 64, "per_launch_bytes": {"k": 1.0}, "source": "s", "rule": "r"}))
    table, src = bench.load_traffic_table()
    assert table == {} and src is None and "different kernel sources" in capsys.readouterr().err
    p.write_text(json.dumps({"csrc_sha256": csrc_hash(), "per_launch_bytes": {"k": 1.0}, "source": "s", "rule": "r"}))
    table, src = bench.load_traffic_table()
    assert table["k"] == 1.0 and "traffic_table.json" in src
    # BASELINE configs 4 / 5 read tables of their own (other shapes, other bytes per launch); any other workload has none
    assert bench.traffic_table_path("") == str(p) and bench.traffic_table_path("config4") == str(tmp_path / "traffic_table_config4.json")
    assert bench.TABLED_WORKLOADS[(128, "bf16", "transdec_postnorm::L4_H1024_A16_F4096", "torchvision::resnet50", 1, 224, 10000)] == "config4"
    assert bench.TABLED_WORKLOADS.get((32, "bf16", "transdec_postnorm::L1_H1024_A16_F4096", "torchvision::resnet50", 1, 224, 10000)) is None
    (tmp_path / "traffic_table_config4.json").write_text(json.dumps({"csrc_sha256": csrc_hash(), "per_launch_bytes": {"k": 2.0}, "source": "s", "rule": "r"}))
    table4, src4 = bench.load_traffic_table(bench.traffic_table_path("config4"))
    assert table4["k"] == 2.0 and "traffic_table_config4.json" in src4
    # a launch family of several instantiations: the focused pass of bench.py times ONE of them, found by launches per step
    p.write_text(json.dumps({"csrc_sha256": csrc_hash(), "per_launch_bytes": {"fam": 300.0, "solo": 7.0}, "source": "s", "rule": "r",
                             "per_kernel": {"fam": {"kern<2>": {"launches_per_step": 47.0, "bytes": 229.0},
                                                    "kern<4>": {"launches_per_step": 4.0, "bytes": 1233.0}}}}))
    table, src = bench.load_traffic_table()
    assert bench.lookup_traffic(table, "fam", 2, 47.0) == (229.0, "kern<2>")
    assert bench.lookup_traffic(table, "fam", 2, 4.2) == (1233.0, "kern<4>")
    assert bench.lookup_traffic(table, "fam", 2, 20.0) == (None, None)          # no instantiation launches that often: no figure
    assert bench.lookup_traffic(table, "fam", 1, None) == (300.0, None)          # the whole family was timed
    assert bench.lookup_traffic(table, "solo", 1, 3.0) == (7.0, None)
    # the class names bench.py derives from the library's profile classes: generation 2 by tile, generation 3 by kernel
    assert bench._kernel_name("[BM = 256, BN = 128, WM = 4, WN = 2, BK = 32, STAGES = 3, AL = vtxg::PlainKC<unsigned short, 2>, "
                              "BL = vtxg::PlainKC<unsigned short, 1>, EP = vtxg::EpiStore<unsigned short, 2>]") == \
        "contraction_v2_kernel<256, 128, 4, 2, PlainKC<bf16, 2>, PlainKC<bf16, 1>, EpiStore<bf16, 2>, 32, 3>"
    assert bench._kernel_name("[BN = 256, AL = vtxg::PlainKC<unsigned short, 4>, BL = vtxg::PlainKC<unsigned short, 4>, "
                              "EP = vtxg::EpiStore<unsigned short>]") == \
        "contraction_v3_256x256_kernel<PlainKC<bf16, 4>, PlainKC<bf16, 4>, EpiStore<bf16, 0>>"
