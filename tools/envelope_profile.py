#!/usr/bin/env python3
"""The stress envelope over load combinations (femshell_combination_envelope) beside what the library offered before it for the
same result: every combination formed on the host, u_c = sum_j f_cj u_j, and sent through femshell_element_resultants, the
envelope taken on the host from the rows.  One MI355X.

Per model and (cases, combinations): wall seconds of both paths, device seconds of the two kernels of the new call and the rate at
which each moves its algorithmic bytes.  One warm-up round, then `rounds` rounds in which the two paths alternate;
medians.  A combination of the old path costs the same whatever its factors are, so a round times `old_combos` of them (all of
them where there are no more) and scales the time to the count of combinations; the output says which.  No threshold: nothing on
the timed path of bench.py runs these kernels.

    python tools/envelope_profile.py [--sizes 141,1414] [--pairs 4x8,8x40,32x256] [--rounds 5] [--old_combos 8]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def old_path(fs, u, factors, t, count):
    """`count` combinations through femshell_element_resultants; the q values from the GLOBAL tensors of a row need the element's
    frame, which the caller does not have: the old path's user took von Mises from words 12, 13 and the principal values from
    the invariants of the 3 x 3 tensors.  Timed: the combination on the host, the call, the invariants, the running extremes."""
    n_cases = len(u)
    best = None
    for c in range(count):
        uc = factors[c, 0] * u[0]
        for j in range(1, n_cases):
            uc += factors[c, j] * u[j]
        rows = fs.element_resultants(uc)
        q = [rows[:, 12], rows[:, 13]]
        for T in (rows[:, 0:6], rows[:, 6:12]):
            tr = T[:, 0] + T[:, 1] + T[:, 2]
            ss = T[:, 0] ** 2 + T[:, 1] ** 2 + T[:, 2] ** 2 + 2.0 * (T[:, 3] ** 2 + T[:, 4] ** 2 + T[:, 5] ** 2)
            r = np.sqrt(np.maximum(0.5 * ss - 0.25 * tr * tr, 0.0))  # in-plane eigenvalues tr / 2 +- r of a tensor of rank two
            q += [0.5 * tr + r, 0.5 * tr - r]
        q = np.stack(q, axis=1)
        if best is None:
            best, who = q, np.zeros(q.shape, np.int32)
        else:
            take = np.where([False, False, False, True, False, True], q < best, q > best)
            best, who = np.where(take, q, best), np.where(take, c, who)
    return best, who


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="141,1414", help="squares per side of the panels (141: 20k nodes, 1414: 4M triangles)")
    ap.add_argument("--pairs", default="4x8,8x40,32x256", help="cases x combinations")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--old_combos", type=int, default=8, help="combinations of the old path timed per round (scaled to all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envelope_ab.txt"))
    args = ap.parse_args()
    from tests.helpers import fullsize

    pkg = importlib.import_module("fem-shell_amd")
    pairs = [tuple(int(v) for v in p.split("x")) for p in args.pairs.split(",")]
    lines = ["# femshell_combination_envelope (new) against n_combos host-side combinations through femshell_element_resultants (old)",
             "# one warm-up round, then %d rounds, the two paths alternating; medians; wall seconds include uploads and downloads" % args.rounds,
             "# old: %d combinations timed per round and scaled to n_combos where there are more (every combination costs the same)" % args.old_combos,
             "# kernel columns: device seconds between events and algorithmic bytes / seconds"]
    for n in (int(v) for v in args.sizes.split(",")):
        m, (nu, E, t) = fullsize.workload("panel", n)
        fs = pkg.FemShell(nu, E, t, device=0)
        fs.set_mesh(m.xyz, m.tri, m.quad)
        lines.append("panel %d x %d squares: %d tri3, %d nodes" % (n, n, len(m.tri), m.n_nodes))
        rng = np.random.default_rng(5)
        for n_cases, n_combos in pairs:
            u = rng.uniform(-1.0, 1.0, (n_cases, m.n_nodes, 6))
            f = rng.uniform(-2.0, 2.0, (n_combos, n_cases))
            count = min(n_combos, args.old_combos)
            new_s, old_s, k1, k2 = [], [], [], []
            for r in range(args.rounds + 1):  # (round 0 warms up)
                t0 = time.perf_counter()
                env, gov, info = fs.combination_envelope(u, f)
                t1 = time.perf_counter()
                old_env, _ = old_path(fs, u, f, t, count)
                t2 = time.perf_counter()
                if r:
                    new_s.append(t1 - t0)
                    old_s.append((t2 - t1) * n_combos / count)
                    k1.append(info["seconds_cases"])
                    k2.append(info["seconds_envelope"])
            if count == n_combos:  # the two paths computed the same envelope
                assert np.allclose(env, old_env, rtol=1e-9, atol=1e-9 * np.abs(env).max())
            mn, mo, m1, m2 = (float(np.median(v)) for v in (new_s, old_s, k1, k2))
            lines.append("  cases %2d combinations %3d  new %.4f s  old %.4f s%s  old / new %.1f   k_case_resultants %.3e s %.3f TB/s   k_envelope %.3e s %.3f TB/s"
                         % (n_cases, n_combos, mn, mo, "" if count == n_combos else " (scaled from %d)" % count, mo / mn, m1,
                            info["bytes_cases"] / m1 / 1e12, m2, info["bytes_envelope"] / m2 / 1e12))
            print(lines[-1], flush=True)
            del u
        fs.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
