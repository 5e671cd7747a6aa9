"""The multi-rank step record on CPU: multigpu.StepAssembler over gloo at world 2 and 3, and the all-devices step entry
(rt_hip_multi_step_loop) without a device.

Every rank takes the FULL problem with N_start = rank, N_parallel = world -- the application's own decomposition
(src/RayTraceImage.cpp:300-313) --, lets the oracle trace its rays into a private cube (tests only: on the GPU the record
comes from a plan in step mode and the cube never exists), reduces it with backend.step_outputs_from_image into the
assembler's buffer and assembles.  What is under test is the buffer layout and the ONE sum-reduce of
raytrace-miniapp_amd/multigpu.py.  Rank 0 must hold the record of the single-rank oracle cube: the same non-negative
terms in another order, hence the reordering bound (n_e + K) 2^-52 per element, an element nothing deposits into exactly
0 (gate_step of tests/test_gpu_step.py)."""
import copy
import importlib
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

from element_gate import counts_from_oracle
from test_gpu_step import gate_step

ROOT = Path(__file__).resolve().parents[1]
rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, name, scale, out_path):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch
    import torch.distributed as dist
    rtw = importlib.import_module("raytrace-miniapp_amd")
    mg = importlib.import_module("raytrace-miniapp_amd.multigpu")
    be = importlib.import_module("raytrace-miniapp_amd.backend")
    from oracle.binding import Oracle

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    full = rtw.scale_problem(rtw.datfile.load(ROOT / "tests" / "golden" / f"{name}.dat.xz"), scale)
    mine = copy.copy(full)
    mine.N_start, mine.N_parallel = rank, world
    assert len(mine.build_rays()) == len(range(rank, full.n_rays_total, world))
    res = Oracle().image_loop(mine)                       # the full beam, this rank's rays
    assert res["failure_code"] == 0
    rec = be.step_outputs_from_image(mine, res["image"])
    a = mg.StepAssembler(full, rank, world)
    b = full.beam
    assert a.buffer.numel() == b.nv + b.nx * b.ny + b.na * b.nb, "(E_v | nf | I_ang), nothing else on these beams"
    assert "none yet" in a.describe() and f"{a.buffer.numel() * 8} B" in a.describe()
    a.E_v.copy_(torch.from_numpy(rec["E_v"]))
    a.nf.copy_(torch.from_numpy(rec["nf"]))
    a.iang.copy_(torch.from_numpy(res["I_ang"]))
    out = a.assemble()
    assert "torch.distributed.reduce(SUM) over gloo" in a.describe() and f"world {world}" in a.describe()
    if rank == 0:
        np.savez(out_path, **{k: v.numpy() for k, v in out.items()})
    else:
        assert out is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name,scale,world", [("ASE_small", 0.2, 2), ("ASE_small", 0.2, 3), ("seed_small", 0.002, 2),
                                              ("seed_small", 0.002, 3)])
def test_step_assembly_matches_the_single_rank_record(tmp_path, oracle, name, scale, world):
    import torch.multiprocessing as mp
    out = tmp_path / "r0.npz"
    mp.spawn(_worker, args=(world, _free_port(), name, scale, str(out)), nprocs=world, join=True)
    got = dict(np.load(out))
    full = rt.scale_problem(rt.datfile.load(ROOT / "tests" / "golden" / f"{name}.dat.xz"), scale)
    want = oracle.image_loop(full)
    assert want["failure_code"] == 0 and np.linalg.norm(want["image"]) > 0
    ref = backend.step_outputs_from_image(full, want["image"])
    ref["I_ang"] = want["I_ang"]
    gate_step(got, ref, full, counts_from_oracle(oracle, full), "reordering", f"StepAssembler over gloo, {name}, world {world}")


def test_step_assembler_world_one_takes_no_collective(ase_small):
    import torch
    mg = importlib.import_module("raytrace-miniapp_amd.multigpu")
    p = rt.scale_problem(ase_small, 0.2)
    a = mg.StepAssembler(p, 0, 1)
    a.buffer.copy_(torch.arange(a.buffer.numel(), dtype=torch.float64))
    out = a.assemble()                                   # (no process group exists: a collective would raise)
    b = p.beam
    assert a.last_collective is None and "none yet" in a.describe()
    assert out["E_v"].numel() == b.nv and out["nf"].numel() == b.nx * b.ny and out["I_ang"].numel() == b.na * b.nb
    assert out["E_v"][0] == 0 and out["nf"][0] == b.nv and out["I_ang"][0] == b.nv + b.nx * b.ny
    assert out["I_ang"].data_ptr() == a.iang_ptr


def test_multi_step_loop_fails_loudly_without_a_device(hip, ase_small):
    lib = backend.HipLibrary.get()
    if lib.device_count() > 0:
        pytest.skip("a GPU is present: the no-device path cannot be shown here")
    with pytest.raises(backend.RayTraceError, match="no HIP device"):
        backend.multi_step_loop(ase_small, ase_small.build_rays()[:64], n_devices=1)
