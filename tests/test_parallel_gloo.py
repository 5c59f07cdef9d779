"""gloo runs (world sizes 2, 3 and 8) of the multi-GPU scheduling (no GPU needed): partitioning + the single collective
per batch, with stand-in per-sequence / per-pair functions so that the expected result is known, and
AccFlow.forward_pair_sharded itself driven with the real 7-frame pair schedule (11 pairs: a 2/1 split over 8 ranks), and the
rotating-root stream mode (run_pair_sharded_stream: equal pair and chain counts per rank over a rotation)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from accflow_amd.networks.AccFlow_ import AccFlow
    from accflow_amd.parallel import deal_pairs, gather_to_root, run_pair_sharded, run_sequence_sharded
    calls = []

    def run_seq(seq):  # "flow of the last frame" stand-in: depends on the sequence only
        calls.append(int(seq[0, 0, 0, 0]))
        return seq.sum(0) * 2.0

    seqs = [torch.full((7, 2, 4, 6), float(i)) + torch.arange(6.0) for i in range(2 * world)]
    out = run_sequence_sharded(run_seq, seqs, dst=0)
    ok = True
    if rank == 0:
        ok &= len(out) == 2 * world and all(torch.equal(o, s.sum(0) * 2.0) for o, s in zip(out, seqs))
    else:
        ok &= out is None
    ok &= sorted(calls) == [2 * rank, 2 * rank + 1]  # each rank touched only its shard
    try:
        run_sequence_sharded(run_seq, seqs[:2 * world - 1], dst=0)
        ok = False
    except ValueError:
        pass

    pairs = AccFlow.pair_schedule(7)
    done = []

    def est(my_pairs):  # 1/8-res "flow" of pair (i, j) = 10*i + j everywhere
        done.extend(my_pairs)
        if not my_pairs:
            return torch.zeros(0, 1, 2, 3, 5)
        return torch.stack([torch.full((1, 2, 3, 5), 10.0 * i + j) for i, j in my_pairs])

    def chain(by_pair):
        return [float(by_pair[p].mean()) for p in pairs]

    # eval_cvo's metric gather with UNEQUAL per-rank sample counts (rank r holds r samples, rank 0 none) and with nothing
    # evaluated anywhere: every rank must leave together
    from accflow_amd.eval_cvo import gather_metrics
    mk = lambda r: [torch.arange(float(r)) + 100.0 * r] if r else []   # noqa: E731
    got = gather_metrics(mk(rank), mk(rank), mk(rank), torch.device("cpu"), world, rank)
    if rank == 0:
        want = torch.cat([torch.arange(float(r)) + 100.0 * r for r in range(1, world)]) if world > 1 else torch.zeros(0)
        ok &= tuple(got.shape) == (3, want.numel()) and torch.equal(got[1], want)
    try:
        gather_metrics([], [], [], torch.device("cpu"), world, rank)
        ok = False
    except SystemExit:
        pass

    res = run_pair_sharded(est, chain, 7, pairs, dst=0)
    if rank == 0:
        ok &= res == [10.0 * i + j for i, j in pairs]
    else:
        ok &= res is None
    from accflow_amd.parallel import deal_for_root
    ok &= [pairs[k] for k in deal_pairs(pairs, world)[rank]] == pairs[rank::world]          # the plain deal = round robin
    ok &= done == [pairs[k] for k in deal_for_root(pairs, world, 0)[rank]]                  # the root swaps to the lightest share
    ok &= len(deal_for_root(pairs, world, 0)[0]) == 11 // world
    ok &= len(pairs) == 11 and len(done) in (11 // world, 11 // world + 1)

    # AccFlow.forward_pair_sharded itself (the method the multi-GPU mode calls) on a stand-in model: the real
    # schedule, the real round-robin deal, the real all_gather, the chain on dst only
    class Stub:
        pair_schedule = staticmethod(AccFlow.pair_schedule)
        seen = []

        def estimate_small(self, images, my_pairs):
            Stub.seen.extend(my_pairs)
            return torch.cat([torch.full((1, 2, 2, 3), 100.0 * i + j) for i, j in my_pairs])

        def fuse_chain(self, images, by_pair):
            return [float(by_pair[p].mean()) for p in AccFlow.pair_schedule(len(images))]

    images = [torch.zeros(1, 3, 16, 24) for _ in range(7)]
    res = AccFlow.forward_pair_sharded(Stub(), images, dst=world - 1)
    if rank == world - 1:
        ok &= res == [100.0 * i + j for i, j in pairs]
    else:
        ok &= res is None
    ok &= Stub.seen == pairs[rank::world]

    # GMA: pairs out of one image1 share an attention matrix and stay on one rank (deal_pairs keep_together)
    class GmaStub(Stub):
        ofe = type("E", (), {"att": object()})()
        seen = []

        def estimate_small(self, images, my_pairs):
            GmaStub.seen.extend(my_pairs)
            return torch.cat([torch.full((1, 2, 2, 3), 100.0 * i + j) for i, j in my_pairs])

    res = AccFlow.forward_pair_sharded(GmaStub(), images, dst=0)
    if rank == 0:
        ok &= res == [100.0 * i + j for i, j in pairs]
    else:
        ok &= res is None
    from accflow_amd.parallel import deal_for_root
    deal = deal_for_root(pairs, world, 0, keep_together=True)       # (the root swaps to the lightest share)
    ok &= GmaStub.seen == [pairs[k] for k in deal[rank]]
    ok &= len(deal[0]) == min(map(len, deal)) and sorted(k for d_ in deal for k in d_) == list(range(len(pairs)))
    for r_, d_ in enumerate(deal):                      # no image1 is split over two ranks
        ok &= all({pairs[k][0] for k in d_}.isdisjoint({pairs[k][0] for k in e_}) for s_, e_ in enumerate(deal) if s_ != r_)
    g = gather_to_root(torch.full((2, 3), float(rank)), dst=0)
    ok &= (g is None) if rank else (len(g) == world and float(g[world - 1].mean()) == world - 1.0)

    # a STREAM of sequences in pair-sharded mode: rotating root + rotated deal (VERDICT r04 #7a).  Over `world` sequences
    # every rank must run the same number of pairs and exactly one chain, and every chain must see all 11 flows of ITS
    # sequence (flow of pair (i, j) of sequence k = 1000 k + 10 i + j).
    from accflow_amd.parallel import rotated_deal, run_pair_sharded_stream
    for gma, with_aux in ((False, False), (True, False), (False, True)):
        did_pairs, did_chain = [], []

        def est_k(seq, my_pairs, is_root):
            did_pairs.extend((int(seq), p_) for p_ in my_pairs)
            flows = (torch.zeros(0, 1, 2, 3, 5) if not my_pairs else
                     torch.stack([torch.full((1, 2, 3, 5), 1000.0 * seq + 10.0 * i + j) for i, j in my_pairs]))
            # aux: a per-rank side value riding in the SAME all_gather (the range-guard flag in AccFlow's stream mode)
            return (flows, torch.tensor([rank, int(seq)], dtype=torch.int32)) if with_aux else flows

        def chain_k(seq, by_pair, aux=None):
            did_chain.append(int(seq))
            if with_aux:        # every rank's aux reached this sequence's root, in rank order
                assert [a_.tolist() for a_ in aux] == [[float(r_), float(seq)] for r_ in range(world)], aux
            else:
                assert aux is None
            return ("pending", [float(by_pair[p_].mean()) for p_ in pairs])     # a handle, resolved by harvest

        nseq = world + (2 if world == 3 else 0)       # (world 3: a stream that is no multiple of the world size)
        res = run_pair_sharded_stream(est_k, chain_k, pairs, list(range(nseq)), keep_together=gma, harvest=lambda h: h[1])
        ok &= sorted(res) == list(range(rank, nseq, world)) == sorted(did_chain)
        ok &= all(res[k] == [1000.0 * k + 10.0 * i + j for i, j in pairs] for k in res)
        if nseq == world:                             # a whole rotation: every share held once -> equal pair counts
            ok &= len(did_pairs) == len(pairs) and len(did_chain) == 1
        for k in range(nseq):                         # the root's share is the lightest; the deal is a partition
            root, deal = rotated_deal(pairs, world, k, keep_together=gma)
            ok &= root == k % world and len(deal[root]) == min(map(len, deal))
            ok &= sorted(i for d_ in deal for i in d_) == list(range(len(pairs)))
            ok &= [p_ for s_, p_ in did_pairs if s_ == k] == [pairs[i] for i in deal[rank]]
    # bounded lag: handles are resolved while the stream runs, never more than two alive per rank; the
    # sequences come from a generator (consumed one at a time) and on_result receives every rooted sequence in order
    alive, peak, got = set(), [0], []

    def chain_l(seq, by_pair, aux=None):
        alive.add(int(seq))
        peak[0] = max(peak[0], len(alive))
        return int(seq)

    def harvest_l(h):
        alive.discard(h)
        return h * 10

    nseq = 4 * world + 1
    res = run_pair_sharded_stream(lambda seq, mp_, root_: (torch.zeros(0, 1, 2, 3, 5) if not mp_ else torch.zeros(len(mp_), 1, 2, 3, 5)),
                                  chain_l, pairs, (k for k in range(nseq)), harvest=harvest_l,
                                  on_result=lambda k, o: got.append((k, o)))
    ok &= res == {} and got == [(k, 10 * k) for k in range(rank, nseq, world)] and 1 <= peak[0] <= 2 and not alive
    q.put((rank, bool(ok)))
    # gloo's own barrier: dist.barrier() asks torch for the machine's accelerator first, which initialises the HIP runtime
    # and opens the GPU in every one of these CPU-only ranks
    dist.monitored_barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(240)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_sequence_and_pair_sharding_gloo(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=200) for _ in procs)
    for p in procs:
        p.join(30)
    assert res == {r: True for r in range(world)}


def test_single_process_paths():
    from accflow_amd.parallel import run_pair_sharded, run_sequence_sharded
    seqs = [torch.ones(3, 2, 2, 2) * i for i in range(3)]
    out = run_sequence_sharded(lambda s: s.mean(0), seqs)
    assert len(out) == 3 and float(out[2].mean()) == 2.0
    pairs = [(2, 1), (2, 0), (1, 0)]
    r = run_pair_sharded(lambda ps: torch.stack([torch.full((1, 2, 2, 2), float(i - j)) for i, j in ps]),
                         lambda bp: {k: float(v.mean()) for k, v in bp.items()}, 3, pairs)
    assert r == {(2, 1): 1.0, (2, 0): 2.0, (1, 0): 1.0}
