#!/usr/bin/env python3
"""Device code of two builds of libfasn.so, kernel by kernel:  tools/kernel_digest.py old.so new.so
For every kernel (FUNC symbol _Z... of the gfx950 code objects): sha256 of its bytes in .text and its resource record (spill_map.kernel_table:
registers, spills, scratch, LDS). Prints the kernels only one side has and the kernels that differ; exit status 1 if a shared kernel differs."""
import hashlib, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spill_map


def digest(lib):
    out, table = {}, spill_map.kernel_table(lib)
    with tempfile.TemporaryDirectory() as td:
        for i, co in enumerate(spill_map.code_objects(lib)):
            f = os.path.join(td, f"co{i}.elf")
            open(f, "wb").write(co)
            secs = subprocess.run([spill_map.READELF, "-S", "-W", f], capture_output=True, text=True, check=True).stdout
            m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", secs)
            addr, off = int(m.group(1), 16), int(m.group(2), 16)
            for line in subprocess.run([spill_map.READELF, "-s", "-W", f], capture_output=True, text=True, check=True).stdout.splitlines():
                p = line.split()
                if len(p) >= 8 and p[3] == "FUNC" and p[7].startswith("_Z"):
                    v, sz = int(p[1], 16), int(p[2])
                    out[p[7]] = (sz, hashlib.sha256(co[off + v - addr: off + v - addr + sz]).hexdigest(), repr(table.get(p[7])))
    return out


def main():
    old, new = digest(sys.argv[1]), digest(sys.argv[2])
    names = spill_map.demangle(sorted(set(old) | set(new)))
    differ = [k for k in old if k in new and old[k] != new[k]]
    for title, ks in (("only in " + sys.argv[1], sorted(set(old) - set(new))), ("only in " + sys.argv[2], sorted(set(new) - set(old))), ("differ", differ)):
        print(f"{title}: {len(ks)}")
        for k in ks:
            print("   ", names.get(k, k))
    print(f"{len(old)} kernels / {sum(v[0] for v in old.values())} bytes -> {len(new)} kernels / {sum(v[0] for v in new.values())} bytes; "
          f"{len(set(old) & set(new)) - len(differ)} shared kernels identical (code bytes and resource record), {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
