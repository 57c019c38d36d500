"""Soak runs of the mutation fuzz (tests/mutation_model.py + tests/test_mutation_fuzz_gpu.py) over seeds outside the suite: the mutation
counterpart of scripts/fuzz_single.py.  One (case, seed) per child process; stops at the first failure and prints its replay line.
Development aid, not part of the suite and not run by bench.py:
    python scripts/fuzz_mutations.py [--cases id,id,...] seed [seed ...]      (seeds: integers, or lo..hi)
    python scripts/fuzz_mutations.py --child case seed                        (what the parent starts)"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(case, seed):
    import pathlib
    from tests import test_mutation_fuzz_gpu as fuzz
    with tempfile.TemporaryDirectory() as tmp:
        fuzz.run_plan(case, pathlib.Path(tmp), seed, cert=case.startswith("cert"), head=case == "head")


def seeds_of(args):
    for a in args:
        if ".." in a:
            lo, hi = a.split("..")
            yield from range(int(lo, 0), int(hi, 0) + 1)
        else:
            yield int(a, 0)


def main(argv):
    if argv[:1] == ["--child"]:
        child(argv[1], int(argv[2], 0))
        return 0
    from tests import mutation_model as mm
    cases = list(mm.CASES)
    if argv[:1] == ["--cases"]:
        cases, argv = argv[1].split(","), argv[2:]
    seeds = list(seeds_of(argv))
    if not seeds:
        print(__doc__)
        return 2
    n = 0
    for seed in seeds:
        for case in cases:
            try:
                mm.plan(case, seed)     # (a seed whose plan cannot be drawn -- no list can be crowded, say -- is skipped, not a failure)
            except AssertionError as e:
                print(f"skip {case} seed {seed:#x}: {e}")
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, hex(seed)], cwd=ROOT, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:])
                print(r.stderr[-6000:])
                print(f"FAILED {case} seed {seed:#x} (exit {r.returncode}) after {n} plans")
                return 1
            n += 1
            print(f"ok {case} seed {seed:#x}: {r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ''}")
    print(f"fuzz_mutations: {n} plans of {mm.STEPS} steps, every step against the Model and the oracle through every search call, bit for bit")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
