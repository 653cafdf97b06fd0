#!/usr/bin/env python3
"""Read / write bytes and L2 (TCC) hits / misses of named kernels per bench window, from the
output directory of tools/profile_round.sh (prof_TAG/{fetch,write}) and, if present, a
counter-only run of the same bench command with the L2 counters in prof_TAG/tcc:

    rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d prof_TAG/tcc -o run -- \
        python3 bench.py --full --queues 2 --steps 20 --warmup 5 --no-cpu-baseline --no-pcie \
        --no-dropin --no-configs

    python tools/pmc_windows.py DIR [DIR ...] [--kernels k_apply k_finish]

Windows as in profiles/summarize.py (40 untimed, 20 timed frames x 2 engines, 3 isolated frames of
engine 0).  Read bytes = 2 x FETCH_SIZE KiB (summarize.py), write bytes = WRITE_SIZE KiB.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
import summarize as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dirs", nargs="+")
    ap.add_argument("--kernels", nargs="+", default=["k_apply", "k_finish"])
    ap.add_argument("--pre", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--queues", type=int, default=2)
    ap.add_argument("--iso", type=int, default=3)
    a = ap.parse_args()
    win = lambda seq: [S.mean(w) for w in S.windows(seq, a.pre, a.steps, a.queues, a.iso)]  # noqa: E731
    print("| run | kernel | read MB timed | read MB isolated | write MB timed | write MB isolated | "
          "TCC hits isolated | TCC misses isolated | hit rate isolated | hit rate timed |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for d in a.dirs:
        fetch = S.pmc(os.path.join(d, "fetch"), "FETCH_SIZE")
        write = S.pmc(os.path.join(d, "write"), "WRITE_SIZE")
        tcc = os.path.isdir(os.path.join(d, "tcc"))
        hit = S.pmc(os.path.join(d, "tcc"), "TCC_HIT_sum") if tcc else {}
        miss = S.pmc(os.path.join(d, "tcc"), "TCC_MISS_sum") if tcc else {}
        for k in sorted(fetch):
            if S.base(k) not in a.kernels:
                continue
            ft, fi = win(fetch[k])
            wt, wi = win(write[k])
            row = [os.path.basename(os.path.normpath(d)), k] + [
                "%.1f" % (x * 1024 / 1e6) for x in (2 * ft, 2 * fi, wt, wi)]
            if k in hit:
                ht, hi = win(hit[k])
                mt, mi = win(miss[k])
                row += ["%.3e" % hi, "%.3e" % mi, "%.3f" % (hi / (hi + mi)), "%.3f" % (ht / (ht + mt))]
            else:
                row += ["-"] * 4
            print("| " + " | ".join(row) + " |")


if __name__ == "__main__":
    main()
