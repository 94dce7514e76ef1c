"""Builds tests/golden/geometry_table.json: per arithmetic configuration a greedy cover of every reachable (launch kind,
bucket) of tests/geometry_checks.py by batch geometries, and the list of the unreachable ones with the reason.  Run it
again when a kernel's tile, a launcher's grid or the dispatch changes (tests/test_geometry_checks_host.py fails then);
the tests read the table, never this search.
    python tools/geometry_cover.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import geometry_checks as G  # noqa: E402

MIXED = (0, 1, 3, 2, 4, 5, 1, 3, 4)            # 11 + 1 + 1 + 9 + 1 + 2 + 1 + 1 + 1 frames: runs of one-frame clips between long ones
ALL = list(range(8, 25))


def order_for(total, pattern):
    """Pool clips, in order, that make `total` frames: `ones` cycles the one-frame clips; `mixed` cycles MIXED and ends in
    one-frame clips where the next clip does not fit."""
    order, have, i = [], 0, 0
    while have < total:
        c = G.ONE_FRAME[i % len(G.ONE_FRAME)] if pattern == "ones" else MIXED[i % len(MIXED)]
        if have + G.POOL_FRAMES[c] > total:
            c = G.ONE_FRAME[i % len(G.ONE_FRAME)]
        order.append(c)
        have += G.POOL_FRAMES[c]
        i += 1
    return order


def candidates():
    for n in range(1, G.MAX_PASS + 1):
        for pattern in ("ones", "mixed"):
            yield dict(order=order_for(n, pattern), fpc=n, frame0=0, nframes=n, tensors=ALL, name="")
        # the tap from frame 3 (inside the first, 11-frame clip) on: a pass of n and one of 5 frames
        if n + 19 <= G.MAX_PASS:
            yield dict(order=order_for(n + 19, "mixed"), fpc=n, frame0=3, nframes=n + 5, tensors=ALL, name="")


def cover(cfg):
    uni, kinds = G.universe(cfg)
    tensor_of = {k: l.tensor for k, l in kinds.items()}
    todo = {p for p, why in uni.items() if why is None}
    cands = [(e, G.entry_cover(cfg, e) & todo) for e in candidates()]
    chosen = []
    while todo:
        def score(c):
            e, hit = c
            new = hit & todo
            tens = {tensor_of[k] for k, _ in new} - {G.HEADS_TENSOR}
            frames = sum(G.POOL_FRAMES[i] for i in e["order"])
            # what a fetch costs on an MI355X: about 2 ms however small, and 0.02 ms per frame (f32: 4 ms and 0.09 ms)
            return len(new) / ((100.0 + frames) * (1 + len(tens)))
        e, hit = max(cands, key=score)
        new = hit & todo
        if not new:
            raise SystemExit("cannot cover: %s" % sorted(todo)[:10])
        e = dict(e, tensors=sorted({tensor_of[k] for k, _ in new} - {G.HEADS_TENSOR}))
        got = G.entry_cover(cfg, e)
        assert new <= got, sorted(new - got)
        todo -= got
        chosen.append(e)
    unreachable = sorted([k, b, why] for (k, b), why in uni.items() if why is not None)
    return chosen, unreachable


def main():
    table = {}
    for name, cfg in G.CONFIGS.items():
        entries, unreachable = cover(cfg)
        frames = sum(sum(G.POOL_FRAMES[i] for i in e["order"]) * (1 + len(e["tensors"])) for e in entries)
        print("%-22s %3d entries, %6d frame-fetches, %d unreachable pairs" % (name, len(entries), frames, len(unreachable)))
        table[name] = {"entries": entries, "unreachable": unreachable}
    with open(G.TABLE_PATH, "w") as f:
        f.write("{\n" + ",\n".join(
            ' %s: {"entries": [\n%s\n ], "unreachable": [\n%s\n ]}' % (
                json.dumps(name), ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in t["entries"]),
                ",\n".join("  " + json.dumps(u) for u in t["unreachable"])) for name, t in table.items()) + "\n}\n")


if __name__ == "__main__":
    main()
