"""Per-kernel summary of the STAMP lines of score_time_iteration (SCORE_TRACE=stamps): workgroups, span from the first entry
to the last exit, median and longest workgroup on the device clock.  The cone launch (kernel 5) is split into its cone
workgroups and its update helpers:   python profiles/scripts/sweep_end_stamps.py <output of a stamps run> <cone workgroups>"""
import statistics
import sys

NAMES = ("rhs", "prec_init", "kp", "prec_step", "kpb", "cone")


def main(path, cone_wgs):
    rows = {}
    for line in open(path):
        if line.startswith("STAMP"):
            _, k, b, t0, t1 = line.split()
            rows.setdefault(int(k), []).append((int(b), float(t0), float(t1)))
    for k in sorted(rows):
        parts = [(NAMES[k], rows[k])]
        if k == 5 and cone_wgs:
            parts = [("cone: cones", [r for r in rows[k] if r[0] < cone_wgs]), ("cone: helpers", [r for r in rows[k] if r[0] >= cone_wgs]),
                     ("cone: launch", rows[k])]
        for name, rs in parts:
            if not rs:
                continue
            d = [t1 - t0 for _, t0, t1 in rs]
            print(f"{name:14s} {len(rs):4d} workgroups  span {max(r[2] for r in rs) - min(r[1] for r in rs):6.2f} us  "
                  f"median {statistics.median(d):5.2f}  longest {max(d):5.2f}  entered at {min(r[1] for r in rs):6.2f}")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0)
