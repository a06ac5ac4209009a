"""One rank of the gathered-store parity run, one PROCESS per rank under torch.distributed.run (tests/test_gpu_shard_f3.py: RCCL, one rank per GPU;
tests/test_dist_gather_cpu.py with `--simt`: the emulated device library and its mailbox transport in RCCL's place): shard a scenario's reads by rank - ragged
shares - build the tables, gather the read store through the transport and compare hao_reads_digest with the definition computed on the host, then every local
read's exact flags, grid pairs, summaries, rescue results and window lists with an unsharded engine over the whole read set in the same process.
Exit code 0 = this rank's store and results are bit-exact."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIG = {"hifi": (775, 0.004), "nn": (200, 0.01)}


def main():
    import torch
    import torch.distributed as dist
    from hifiasm_amd.api import Engine
    from hifiasm_amd import shard
    from helpers import scenario_reads
    import test_gpu_shard_f3 as S
    name = sys.argv[1]
    simt = "--simt" in sys.argv[2:]
    rank, world, lr = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    if simt:
        import simt_build
        from hifiasm_amd import api
        path = simt_build.build_lib(); api.lib_path = lambda: path; api._LIB = None
        dist.init_process_group("gloo", rank=rank, world_size=world)
        lr = 0
    else:
        torch.cuda.set_device(lr)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", lr))
    rs, okw = scenario_reads(name)
    wl, e_rate = CONFIG[name]
    cuts = S._cuts(rs.n, world) if world in (2, 3) else [rs.n * i // world for i in range(world + 1)]
    lo, hi = cuts[rank], cuts[rank + 1]
    e = Engine(lr, **okw)
    e.set_readset(S._shard(rs, lo, hi))
    all_len, counts = shard.gather_lengths(dist, rs.lengths[lo:hi].copy(), device="cpu" if simt else "cuda")
    assert (all_len == rs.lengths).all()
    e.set_shard(sum(counts[:rank]), all_len)
    e.dist_init(shard.share_unique_id(dist, Engine.dist_unique_id), rank, world)
    e.ha_ft_gen(); e.ha_pt_gen()
    e.dist_gather_reads()
    dg = e.reads_digest()
    assert dg == S._host_digest(rs), (dg, S._host_digest(rs))
    got, _ = S._blocking(e, hi - lo, lo, wl, e_rate)
    e.close()
    u = Engine(lr, **okw)                                        # the unsharded engine over the same reads (no transport)
    u.set_readset(rs); u.ha_ft_gen(); u.ha_pt_gen()
    want, _ = S._blocking(u, rs.n, 0, wl, e_rate)
    u.close()
    bad = [(r, S._diff(got[r], want[r])) for r in range(lo, hi) if S._diff(got[r], want[r]) is not None]
    n_rec = sum(x[0].shape[0] for r in range(lo, hi) for x in got[r]["wl"])
    dist.barrier()
    dist.destroy_process_group()
    print(f"[gather_worker] rank {rank}/{world} {name}: {hi - lo} reads, {n_rec} window records, {len(bad)} differ {bad[:3]}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
