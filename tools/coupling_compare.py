"""developer probe: compare `tools/coupling_launches.py --dump` files of two builds.
python tools/coupling_compare.py PARENT_1.pt PARENT_2.pt [PARENT_3.pt ...] -- NEW_1.pt [NEW_2.pt ...]
Forward outputs (z, nll, sample: no float atomics) must be bit-identical (torch.equal) between every new and every parent
file.  Gradients pass through float atomics: per parameter group (the parameter's name without its layer's position
in the flow) the largest absolute difference of any new file against any parent file stands beside the parent's own pairs,
their largest and smallest, and the largest of the new build's own pairs; `ok` = new-vs-parent <= largest parent pair +
(largest - smallest parent pair), the parent's run-to-run variation.  Exit status 1 if a forward output differs or a
group is not ok."""
import itertools, re, sys
import torch

sep = sys.argv.index("--")
parents = [torch.load(f) for f in sys.argv[1:sep]]
news = [torch.load(f) for f in sys.argv[sep + 1:]]
assert len(parents) >= 2 and news
bad = 0
for case in parents[0]:
    print("== %s: %d parent files (%d pairs), %d new" % (case, len(parents), len(parents) * (len(parents) - 1) // 2, len(news)))
    for key in ("z", "nll", "sample"):
        same = all(torch.equal(n[case][key], p[case][key]) for n in news for p in parents)
        bad += not same
        print("%-8s new == parent bitwise: %s   (parent == parent: %s)" % (
            key, same, all(torch.equal(a[case][key], b[case][key]) for a, b in itertools.combinations(parents, 2))))
    groups = {}
    for key in parents[0][case]:
        if key.startswith("grad/"):
            groups.setdefault(re.sub(r"\.\d+\.", ".*.", key[5:], count=1), []).append(key)
    print("%-44s %10s %12s %12s %12s %12s  %s" % ("gradient group", "max |g|", "new-parent", "pp largest", "pp smallest",
                                                  "new-new", "ok"))
    for grp, keys in sorted(groups.items()):
        def worst(a, b):
            return max(float((a[case][k] - b[case][k]).abs().max()) for k in keys)
        pp = [worst(a, b) for a, b in itertools.combinations(parents, 2)]
        nw = max(worst(n, p) for n in news for p in parents)
        nn = max([worst(a, b) for a, b in itertools.combinations(news, 2)], default=float("nan"))
        ok = nw <= max(pp) + (max(pp) - min(pp))
        bad += not ok
        print("%-44s %10.3e %12.3e %12.3e %12.3e %12.3e  %s" % (
            grp, max(float(parents[0][case][k].abs().max()) for k in keys), nw, max(pp), min(pp), nn, ok))
sys.exit(1 if bad else 0)
