"""One rank of the index-file run between PROCESSES, one process per rank under torch.distributed.run (tests/test_dist_indexfile_cpu.py with `--simt`: the
emulated device library and its mailbox transport in RCCL's place; without it: RCCL, one rank per GPU).  Shard a scenario's reads by rank - ragged shares -
build the tables, gather the read store and save: a collective in which rank 0 writes and the others learn the result.  The moment its own call returns, every
rank compares the three files with those an unsharded engine over the whole read set writes in the same process - so a rank's return has waited for rank 0's
write.  Then the world loads the files back with the same cuts and every rank compares its reads' overlaps, fake cigars and chained hits with the oracle's.
Exit code 0 = this rank's files and results are bit-exact."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SUFFIXES = (".pt_flt", ".pt_flt.bin", ".pt_flt.paf.bin")


def main():
    import torch
    import torch.distributed as dist
    from hifiasm_amd.api import Engine
    from hifiasm_amd import shard
    from helpers import scenario_reads, scenario_oracle
    import test_gpu_shard_f3 as S
    name, out_dir = sys.argv[1], sys.argv[2]
    simt = "--simt" in sys.argv[3:]
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
    cuts = S._cuts(rs.n, world) if world in (2, 3) else [rs.n * i // world for i in range(world + 1)]
    lo, hi = cuts[rank], cuts[rank + 1]
    u = Engine(lr, **okw)                                        # the unsharded engine over the same reads (no transport): the files to expect
    u.set_readset(rs); u.ha_ft_gen(); u.ha_pt_gen()
    u.index_save(os.path.join(out_dir, f"one{rank}"))
    u.close()
    want = [open(os.path.join(out_dir, f"one{rank}") + s, "rb").read() for s in SUFFIXES]
    e = Engine(lr, **okw)
    e.set_readset(S._shard(rs, lo, hi)); e.set_shard(lo, rs.lengths)
    e.dist_init(shard.share_unique_id(dist, Engine.dist_unique_id), rank, world)
    e.ha_ft_gen(); e.ha_pt_gen()
    e.dist_gather_reads()
    prefix = os.path.join(out_dir, "world")
    e.index_save(prefix)
    got = [open(prefix + s, "rb").read() for s in SUFFIXES]      # (nothing between the call's return and the read)
    bad = [s for s, a, b in zip(SUFFIXES, got, want) if a != b]
    dist.barrier()                                               # (everybody has read the files: rank 0 may go on)
    assert e.index_load(prefix, cuts) == 3
    assert (e.rid_base, e.n_reads) == (lo, hi - lo)
    e.overlap_batch(0, hi - lo)
    o = scenario_oracle(name)
    for r in range(lo, hi):
        ol, fc, fo, cl = e.h_ec_lchain(r - lo)
        ool, ofc, ofo, ocl = o.lchain(r)
        if not (ol.shape == ool.shape and (ol == ool).all() and (fc == ofc).all() and cl.shape == ocl.shape and (cl == ocl).all()):
            bad.append(r)
    e.close()
    dist.barrier()
    dist.destroy_process_group()
    print(f"[indexfile_worker] rank {rank}/{world} {name}: {sum(len(x) for x in got)} bytes in 3 files, {hi - lo} reads, {len(bad)} differ {bad[:3]}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
