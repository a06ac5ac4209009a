"""hao_dist_gather_reads between PROCESSES on the CPU: 2 and 3 ranks under torch.distributed.run, the emulated device library (tests/simt) in every process and
tests/simt/rccl/rccl.h - the mailbox transport - in RCCL's place, so what runs is hao_comm_allgatherv's RCCL branch under the chunked gather (tests/gather_worker.py:
every rank compares hao_reads_digest with the definition and its reads' window lists - and what leads to them - with an unsharded engine; exit code 0 = bit-exact).
The second case lowers the chunk to 4 KB: the broadcast-per-root branch of lopsided exchanges and the padded all-gather both run many times."""
import os
import socket
import subprocess
import sys

import pytest


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


@pytest.mark.parametrize("name,world,env", [("hifi", 2, {}), ("nn", 3, {"HAO_DBG_TEST": "gather_chunk=4096"})])
def test_gather_between_processes(name, world, env):
    import simt_build
    simt_build.build_lib()      # once, before the ranks start (they would otherwise queue on the build lock)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(root, "tests", "gather_worker.py"), name, "--simt"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=dict(os.environ, OMP_NUM_THREADS="1", HAO_SIMT_RCCL_TIMEOUT="600", **env))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count("0 differ") == world, r.stdout[-1500:]
