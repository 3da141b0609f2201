#!/usr/bin/env python3
"""The agglomeration of the fragment graph on the device (include/pea_agglo.h: pea_agglo_merge), timed in ONE process at three shapes
against what the loop's waterz path has to do today with a region adjacency graph that is on the device:

  merge        pea.agglomerate_graph(rag, threshold=0.5, rounds=R) on the RAG's device tables, R = the rounds that the data needs
               (found once with rounds=None) + 1: the launches of csrc/pea_k_agglo.hip, nothing read back
  merge_auto   the same with rounds=None: batches of 32, 64, .. rounds with one synchronisation each, the tables sized from the edge count
  chain        pea.region_adjacency(.., max_id, capacity, max_edges) + merge + pea.project_node_labels: fragments and affinities in,
               segmentation out, no synchronisation
  default_chain  the same with nothing named, as seg_waterz and pea.agglomerate call it: a FRESH RAG of default size per repetition
               (fragments.max() read back), rounds=None (the RAG's stats and one word per batch of rounds read back), the projection
  host         device -> host copy of the RAG's tables (uv, mean, count), the sequential procedure "pop the cheapest live edge, merge
               while below the threshold, rescore" with a heap in numpy / Python, the node labels copied back.  waterz is not installed
               here, so this is NOT waterz's own time: its loop is compiled code, this one is interpreted.  It says what THIS machine's
               caller pays.  Skipped above --host-max-edges edges.

  2d_1x520x696         one BBBC039V1-sized image, offsets (-1, 0), (0, -1)
  ac3_2x18x160x160     two AC3/AC4 validation blocks
  ac3_1x100x1024x1024  one full AC3/AC4 volume

The maps are affinities of Voronoi cells (utils/synth.py synth_membranes; a volume's planes are windows of one plane shifted by one
pixel per plane) with walls two pixels thick, in two kinds: "trained" = 0.8 * same + 0.1 + 0.1 * uniform and "noisy" = 0.4 * same + 0.6 * uniform.  The fragments are
the package's distance-transform watershed (threshold .25, sigma_seeds 2) of the boundary map, plane by plane.  Recorded: the rounds
used, the edges at the start and at the end, and the time per round in the first and in the second half of the rounds (device events
around calls with 0, R / 2 and R rounds).  Medians by alternating batches with their min and max; a batch repeats its call until the
timed window is at least --window-ms long (at least --reps times); recorded, not gated.

  python profiles/agglo_ab.py [--batches 5] [--reps 3] [--window-ms 30] [--warmup 2] [--out profiles/agglo_ab.json] [--only LEG] [--no-host]"""
import argparse
import heapq
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LEGS = {"2d_1x520x696": dict(B=1, dims=(1, 520, 696), cells=300),
        "ac3_2x18x160x160": dict(B=2, dims=(18, 160, 160), cells=25),
        "ac3_1x100x1024x1024": dict(B=1, dims=(100, 1024, 1024), cells=900)}
THRESHOLD = 0.5


def make_affs(synth, kw, kind, dev, seed=93):
    """float32 [B, ndim, (Z,) Y, X] on the device"""
    B, (Z, Y, X) = kw["B"], kw["dims"]
    _, cells = synth.synth_membranes(B, Y + Z, X + Z, kw["cells"], seed=seed)
    cells = torch.from_numpy(cells).to(dev)
    lab = torch.stack([torch.stack([cells[b, z:z + Y, z:z + X] for z in range(Z)]) for b in range(B)])
    nd = 2 if Z == 1 else 3
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    out = torch.zeros((B, nd, Z, Y, X), dtype=torch.float32, device=dev)
    # a wall is two pixels thick, as a network draws it: the pixels with an in-plane neighbour of another cell.  With one-pixel walls the
    # flood puts a fragment's border beside the wall, where every crossing sample says "same", and every threshold merges everything
    wall = torch.zeros((B, Z, Y, X), dtype=torch.bool, device=dev)
    for ax in (2, 3):
        differ = lab.narrow(ax, 1, lab.shape[ax] - 1) != lab.narrow(ax, 0, lab.shape[ax] - 1)
        wall.narrow(ax, 1, lab.shape[ax] - 1).logical_or_(differ)
        wall.narrow(ax, 0, lab.shape[ax] - 1).logical_or_(differ)
    for k in range(nd):
        ax = k + (3 - nd) + 1
        same = torch.zeros((B, Z, Y, X), dtype=torch.float32, device=dev)
        sl_p = [slice(None)] * 4
        sl_q = [slice(None)] * 4
        sl_p[ax], sl_q[ax] = slice(1, None), slice(0, -1)
        eq = lab[tuple(sl_p)] == lab[tuple(sl_q)]
        if ax != 1:  # in-plane channels are low all over the wall; z joins equal cells
            eq = eq & ~wall[tuple(sl_p)]
        same[tuple(sl_p)] = eq.float()
        u = torch.rand((B, Z, Y, X), generator=gen, device=dev)
        out[:, k] = 0.4 * same + 0.6 * u if kind == "noisy" else 0.8 * same + 0.1 + 0.1 * u
    return out[:, :, 0] if nd == 2 else out


def host_sequential(uv, mean, count, n_nodes, thr):
    """the sequential procedure with a lazy-deletion heap: -> root [n_nodes].  Payload (sum, count) in float64: a restatement for the
    clock, not the header's fixed point"""
    nbr = [dict() for _ in range(n_nodes)]
    for (u, v), m, c in zip(uv.tolist(), mean.tolist(), count.tolist()):
        if u == 0 or c == 0:
            continue
        nbr[u][v] = nbr[v][u] = (m * c, c)
    heap = [(np.float32(s / c), u, v) for u in range(n_nodes) for v, (s, c) in nbr[u].items() if u < v]
    heapq.heapify(heap)
    parent = list(range(n_nodes))
    thr = np.float32(thr)
    while heap:
        sc, u, v = heapq.heappop(heap)
        if not sc < thr:
            break
        e = nbr[u].get(v)
        if parent[u] != u or parent[v] != v or e is None or np.float32(e[0] / e[1]) != sc:
            continue  # stale
        a, b = (u, v) if u < v else (v, u)
        parent[b] = a
        del nbr[a][b]
        for w, (s, c) in nbr[b].items():
            if w == a:
                continue
            del nbr[w][b]
            if w in nbr[a]:
                s0, c0 = nbr[a][w]
                s, c = s + s0, c + c0
            nbr[a][w] = nbr[w][a] = (s, c)
            heapq.heappush(heap, (np.float32(s / c), min(a, w), max(a, w)))
        nbr[b] = {}
    root = np.arange(n_nodes)
    for i in range(n_nodes):
        r = i
        while parent[r] != r:
            r = parent[r]
        root[i] = r
    return root


def event_time(f, reps):
    t = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return statistics.median(t[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-max-edges", type=int, default=400000)
    ap.add_argument("--only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agglo_ab.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "agglo_ab.py measures on an MI355X: there is no CPU fallback"
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    dev = torch.device("cuda:0")
    rows = {}
    for name, kw, kind in [(n, k, kind) for n, k in LEGS.items() for kind in ("trained", "noisy")]:
        if a.only and a.only != name:
            continue
        A = make_affs(synth, kw, kind, dev)
        B, nd = kw["B"], A.dim() - 2
        offs = [[-1 if i == k else 0 for i in range(nd)] for k in range(nd)]
        i, j = (1, 2) if nd == 3 else (0, 1)
        frag = torch.stack([pkg.distance_transform_watershed(torch.maximum(1 - A[b, i], 1 - A[b, j]).contiguous(), .25, 2.)[0] for b in range(B)])
        max_id = int(frag.max())
        rag = pkg.region_adjacency(frag, A, offs, one_minus=True, ignore_zero=True, max_id=max_id, batched=True)
        n_edges = rag.n_edges
        cap, me = rag.capacity, rag.max_edges
        auto = pkg.agglomerate_graph(rag, threshold=THRESHOLD, ignore_zero=True)
        st = auto.stats.cpu().numpy()
        rounds = int(st[:, 0].max()) + 1  # (+ 1: the round that finds nothing left and says so)
        fixed = pkg.agglomerate_graph(rag, threshold=THRESHOLD, ignore_zero=True, rounds=rounds)
        assert fixed.complete and torch.equal(fixed.root, auto.root)

        def chain():
            r = pkg.region_adjacency(frag, A, offs, one_minus=True, ignore_zero=True, max_id=max_id, capacity=cap, max_edges=me, batched=True)
            out = pkg.agglomerate_graph(r, threshold=THRESHOLD, ignore_zero=True, rounds=rounds)
            return [pkg.project_node_labels(frag[b], out.labels[b]) for b in range(B)]

        def default_chain():  # what a caller of seg_waterz / pea.agglomerate pays: a fresh RAG of default size, nothing named
            r = pkg.region_adjacency(frag, A, offs, one_minus=True, ignore_zero=True, batched=True)
            out = pkg.agglomerate_graph(r, threshold=THRESHOLD, ignore_zero=True)
            return [pkg.project_node_labels(frag[b], out.labels[b]) for b in range(B)]

        steps = {"merge": lambda: pkg.agglomerate_graph(rag, threshold=THRESHOLD, ignore_zero=True, rounds=rounds),
                 "merge_auto": lambda: pkg.agglomerate_graph(rag, threshold=THRESHOLD, ignore_zero=True), "chain": chain,
                 "default_chain": default_chain}
        reps = {}
        for v, f in steps.items():
            for _ in range(a.warmup):
                f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            # a timed window of at least --window-ms: a call of half a millisecond is repeated some sixty times per batch
            reps[v] = max(a.reps, min(256, int(a.window_ms * 1e-3 / max(1e-6, time.perf_counter() - t0)) + 1))
        times = {v: [] for v in steps}
        for _ in range(a.batches):
            for v, f in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps[v]):
                    f()
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e6 / reps[v])
        row = {v: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t), "reps_per_batch": reps[v]} for v, t in times.items()}
        ev_reps = max(a.reps, min(32, reps["merge"] // 4))
        t0_, th_, tr_ = (event_time(lambda r=r: pkg.agglomerate_graph(rag, threshold=THRESHOLD, ignore_zero=True, rounds=r), ev_reps) for r in (0, rounds // 2, rounds))
        row["device_split"] = {"setup_and_outputs_us": t0_, "rounds_us": tr_ - t0_, "us_per_round_first_half": (th_ - t0_) / max(1, rounds // 2),
                               "us_per_round_second_half": (tr_ - th_) / max(1, rounds - rounds // 2), "launches": 2 + 5 * rounds + 7}
        row["values"] = {"fragments_max_id": max_id, "edges_at_start": n_edges, "edges_at_end": st[:, 1].tolist(), "rounds_used_per_image": st[:, 0].tolist(),
                         "rounds_enqueued": rounds, "merges": st[:, 3].tolist(), "clusters": st[:, 4].tolist(), "rag_capacity": cap, "rag_max_edges": me,
                         "threshold": THRESHOLD}
        if not a.no_host and max(n_edges) <= a.host_max_edges:
            host_t = []
            for _ in range(5 if max(n_edges) <= 20000 else 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t = rag.tensors
                uv, mean, count, stats = t["uv"].cpu().numpy(), t["mean"].cpu().numpy(), t["count"].cpu().numpy(), t["stats"].cpu().numpy()
                roots = [host_sequential(uv[b, :stats[b, 0]], mean[b, :stats[b, 0]], count[b, :stats[b, 0]], max_id + 1, THRESHOLD) for b in range(B)]
                back = torch.from_numpy(np.stack(roots)).to(dev)
                torch.cuda.synchronize()
                host_t.append((time.perf_counter() - t0) * 1e6)
            row["host"] = {"us": statistics.median(host_t), "min_us": min(host_t), "max_us": max(host_t), "reps": len(host_t)}
            row["values"]["root_equal_host"] = bool(torch.equal(back.to(torch.int32), auto.root))
            row["host_over_merge"] = row["host"]["us"] / row["merge"]["median_us"]
        elif not a.no_host:
            row["host"] = {"skipped": "%d edges exceed --host-max-edges %d" % (max(n_edges), a.host_max_edges)}
        row["shape"] = list(A.shape)
        rows[name + "/" + kind] = row
        print(name, kind, json.dumps(row), flush=True)
        del A, frag, rag, auto, fixed
        torch.cuda.empty_cache()
    out = {"kernel_form": "a lane per table slot, two open-addressing tables of the live edges keyed by the root pair (four words a slot), five launches "
                          "a round (best / merge / compress / re-key / flip), a wave peels its keys before it claims slots; no compaction of the "
                          "table as the edges become fewer (csrc/pea_k_agglo.hip)",
           "host_path": "device -> host copy of uv, mean, count; the sequential procedure with a lazy-deletion heap in Python; host -> device copy "
                        "of the roots.  waterz is not installed on the measuring machine: this is not waterz's own time",
           "timing": "host clock around calls that end in a device synchronise, medians over alternating batches; device_split: device events "
                     "around Python calls with 0, R / 2 and R rounds, medians",
           "batches": a.batches, "min_reps_per_batch": a.reps, "window_ms": a.window_ms, "warmup": a.warmup, "us_per_call": rows, "device": torch.cuda.get_device_name(0)}
    if a.out and not a.only:
        json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
