"""CPU, world_size 2, gloo: the only N > 1 logic of this path.  The GEMM path does not shard (replicas
only, no data-path collective); bench.py --gpus N runs N independent replicas and uses torch.distributed just for the
barriers and the max-over-ranks of the timed region.  This test runs that reduction over gloo in two processes.
The last two tests cover the benchmark's --dump-outputs file (CPU) and a plain single-GPU run end to end (GPU)."""
import os
import socket
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_max_over_ranks_and_aggregate_with_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(textwrap.dedent(f"""
        import os, sys
        sys.path.insert(0, {ROOT!r})
        import torch.distributed as dist
        import bench
        dist.init_process_group("gloo")
        rank = dist.get_rank()
        dist.barrier()
        wall = bench.max_over_ranks(0.010 * (rank + 1))          # rank 1 is the slow replica
        val = bench.aggregate_value(2.0 * 4096 ** 3, 10, dist.get_world_size(), wall)
        print(f"RESULT rank={{rank}} wall={{wall:.6f}} value={{val:.3f}}", flush=True)
        dist.barrier()
        dist.destroy_process_group()
    """))
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    want_wall = 0.020
    want_val = 2.0 * 4096 ** 3 * 10 * 2 / want_wall / 1e12
    for out in outs:
        line = [l for l in out.splitlines() if l.startswith("RESULT")][0]
        kv = dict(t.split("=") for t in line.split()[1:])
        assert abs(float(kv["wall"]) - want_wall) < 1e-9 and abs(float(kv["value"]) - want_val) < 1e-3, line


def test_single_process_is_identity():
    sys.path.insert(0, ROOT)
    import bench

    assert bench.max_over_ranks(0.5) == 0.5
    assert abs(bench.aggregate_value(2.0 * 4096 ** 3, 200, 1, 200 * 40e-6) - 2.0 * 4096 ** 3 / 40e-6 / 1e12) < 1e-6


def test_dump_outputs_writes_a_fixed_float32_row_sample(tmp_path):
    """--dump-outputs: a seeded row sample of the (M, N) bf16 output as float32 (bf16 -> float32 is exact), the same rows every time, under 64 MB."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    out = torch.arange(bench.M * bench.N, dtype=torch.float32).remainder_(251.0).sub_(125.0).view(bench.M, bench.N).to(torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out)
    got, again = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    rows = np.sort(np.random.default_rng(0).choice(bench.M, bench.DUMP_ROWS, replace=False))
    assert got.dtype == np.float32 and got.shape == (bench.DUMP_ROWS, bench.N)
    assert np.array_equal(got, out.float().numpy()[rows]) and np.array_equal(got, again)
    assert os.path.getsize(tmp_path / "a" / "out.npy") <= 64 * 10 ** 6


@pytest.mark.gpu
def test_plain_run_times_exactly_the_steps_and_dumps_the_last_output(tmp_path):
    """A plain `bench.py` run (no --full): the headline line with `steps` = --steps and no side measurements, and DIR/out.npy holds what the timed path
    returned -- bit for bit the product path on the same seeded operands, and the oracle's bits on a few of its rows."""
    import json

    import numpy as np
    import torch

    import oracle
    import qutlass_amd
    from qutlass_amd.utils import to_blocked

    sys.path.insert(0, ROOT)
    import bench

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["unit"] == "TFLOP/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] - 2.0 * bench.M * bench.N * bench.K / (line["ms_per_step"] * 1e-3) / 1e12) <= 0.01 * line["value"]
    assert line["cpu_baseline"] is None and "configs" not in line and "power" not in line and line["roofline"]["per_launch_us"] is None
    got = np.load(tmp_path / "out.npy")
    assert got.dtype == np.float32 and got.shape == (bench.DUMP_ROWS, bench.N)

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    a = torch.randn(bench.M, bench.K, dtype=torch.bfloat16, device=dev) * 25.0
    b = torch.randn(bench.N, bench.K, dtype=torch.bfloat16, device=dev) * 25.0
    h = bench.hadamard(32, dev)
    a_q, a_s = qutlass_amd.fusedQuantizeMx(a, h, method="abs_max")
    b_q, b_s = qutlass_amd.fusedQuantizeMx(b, h, method="abs_max")
    want = qutlass_amd.matmul_mxf4_bf16_tn(a_q, b_q, to_blocked(a_s), to_blocked(b_s), torch.tensor([1.0], device=dev))
    rows = np.sort(np.random.default_rng(0).choice(bench.M, bench.DUMP_ROWS, replace=False))
    assert np.array_equal(got, want[torch.from_numpy(rows).to(dev)].float().cpu().numpy())
    few = [int(rows[0]), int(rows[len(rows) // 2]), int(rows[-1])]
    ri = torch.tensor(few, device=dev)
    k32 = bench.K // 32
    a_s_rm = a_s.cpu().view(torch.uint8).numpy().reshape(-1)[: bench.M * k32].reshape(bench.M, k32)
    b_s_rm = b_s.cpu().view(torch.uint8).numpy().reshape(-1)[: bench.N * k32].reshape(bench.N, k32)
    ref = oracle.gemm_blockscaled(oracle.KIND_MXFP4, a_q[ri].cpu().numpy(), b_q.cpu().numpy(), oracle.to_blocked(np.ascontiguousarray(a_s_rm[few])),
                                  oracle.to_blocked(b_s_rm), 1.0, len(few), bench.N, bench.K)
    assert np.array_equal(got[np.searchsorted(rows, few)], oracle.bf16_bits_to_f32(ref))
