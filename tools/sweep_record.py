"""Records tests/golden/sweep_recorded.json: what the sorted sweep's batches of tests/sweep_recorded.py leave behind -- the result
summary, a digest of fetch(), launches and algorithmic bytes of the locate, partition, resolve, expand and sort kernel classes -- at
the commit checked out, for tests/test_gpu_sweep_recorded.py to replay at every later one.

    python tools/sweep_record.py --commit <name of the commit checked out>      every group twice, each in a fresh process; writes the fixture
    python tools/sweep_record.py --group wide                                    one group in this process; its observations as one JSON line

A field that differs between the two recordings is left out of the fixture and named under "unstable"."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sweep_recorded as S      # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "sweep_recorded.json")


def observe_group(group):
    os.environ.update(S.GROUP_ENV.get(group, {}))
    import vlg_matching_amd as V
    V.lib()
    return {name: run() for name, run in S.cases(V, group).items()}


def observe_group_in_child(group):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--group", group]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError("group %s failed (rc %d):\n%s" % (group, out.returncode, (out.stdout + out.stderr)[-4000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", choices=S.GROUPS)
    ap.add_argument("--commit")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    if args.group:
        print(json.dumps(observe_group(args.group)))
        return
    if not args.commit:
        ap.error("--commit: the fixture names the commit it was recorded at")
    a, b = ({name: obs for g in S.GROUPS for name, obs in observe_group_in_child(g).items()} for _ in range(2))
    unstable = []
    for name in a:
        for part in a[name]:
            for field in list(a[name][part]):
                if a[name][part][field] != b[name][part][field]:
                    unstable.append("%s: %s.%s" % (name, part, field))
                    del a[name][part][field]
    with open(args.out, "w") as f:
        json.dump({"recorded_at": args.commit, "recorded_by": "tools/sweep_record.py", "unstable": unstable, "cases": a}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d unstable fields -> %s" % (len(a), len(unstable), args.out))


if __name__ == "__main__":
    main()
