"""hao_index_save and hao_index_load_dist between PROCESSES on the CPU: 2 ranks under torch.distributed.run, the emulated device library (tests/simt) in every
process and tests/simt/rccl/rccl.h - the mailbox transport - in RCCL's place (tests/indexfile_worker.py: the world saves, every rank compares the files with a
single-process engine's the moment its own call returns - rank 1's return has to wait for rank 0's write - then the world loads them back and every rank
compares its reads' results with the oracle's; exit code 0 = bit-exact).  The only place where "rank 0 writes, the others learn the result" runs between
processes: the loopback worlds of tests/test_gpu_shard_indexfile.py share one address space."""
import os
import socket
import subprocess
import sys
import tempfile


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def test_index_files_between_processes():
    import simt_build
    simt_build.build_lib()      # once, before the ranks start (they would otherwise queue on the build lock)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tempfile.mkdtemp(prefix="hao_didx_")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(root, "tests", "indexfile_worker.py"), "nn", d, "--simt"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=dict(os.environ, OMP_NUM_THREADS="1", HAO_SIMT_RCCL_TIMEOUT="600"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count("0 differ") == 2, r.stdout[-1500:]
