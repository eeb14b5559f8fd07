"""Turns the remarks of -Rpass-analysis=kernel-resource-usage (a build log on stdin or the files named) into one sorted line a
kernel: name, VGPRs, AGPRs, SGPRs, scratch, occupancy, spills, LDS.  Two builds' tables are compared with diff(1): that is how
profiles/soft_resource_usage.txt shows that a change to shared code left every existing kernel as it was.

A parallel build interleaves the units' remarks; a kernel's own lines still follow its name in order, and a block that does
not, or a line that two units wrote into one another, is reported instead of being guessed at (exit status 1): compile
those units again with a log of their own and name that log too -- a kernel read twice must read the same."""
import fileinput
import re
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
REMARK = re.compile(r"^(\S+?):\d+:\d+: remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]\s*$")


def main():
    open_blocks, done, broken = {}, {}, 0            # per source position: the kernel whose lines are arriving
    for line in fileinput.input():
        m = REMARK.match(line)
        if not m:
            broken += 1 if "remark:" in line else 0     # two units' lines written into one another
            continue
        where, text = m.group(1), m.group(2)
        if text.startswith("Function Name:"):
            if where in open_blocks:
                broken += 1
            open_blocks[where] = (text.split(":", 1)[1].strip(), {})
            continue
        if where not in open_blocks or ":" not in text:
            continue
        key, value = (t.strip() for t in text.rsplit(":", 1))
        name, got = open_blocks[where]
        got[key] = value
        if key == FIELDS[-1]:
            if name in done and done[name] != got:
                print("%s: two different blocks" % name, file=sys.stderr)
                broken += 1
            done[name] = got
            del open_blocks[where]
    broken += len(open_blocks)
    for name in sorted(done):
        print(name + "  " + "  ".join("%s %s" % (k.split(" [")[0], done[name].get(k, "?")) for k in FIELDS))
    if broken:
        print("%d block(s) could not be read" % broken, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
