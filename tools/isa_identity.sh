#!/bin/bash
# tools/isa_identity.sh TREE_A TREE_B [OUT.json] — is the device code of two checkouts the same?  No GPU needed.
# Every file of the Makefile's HIP_SRCS is compiled to device-only assembly with the Makefile's flags (k_pcm.hip with
# -ffp-contract=off); comment, debug and .ident lines are dropped; per file: identical or not, and per kernel of each
# tree: vgpr_count, sgpr_count, private_segment_fixed_size and the instruction line count.  Sources and flags are read
# from each tree's own Makefile (HIP_SRCS, CXXFLAGS); EXTRA="-D..." adds flags as `make EXTRA=...` does.
# Where a file differs (say, B instantiates a kernel template more often, or with one more parameter), "a_kernels_in_b" names for
# every kernel of A the kernel of B whose body and .amdhsa_kernel block are A's line for line once each one's own mangled name is
# set aside (null: none).
set -euo pipefail
A=$1; B=$2; OUT=${3:-/dev/stdout}; HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}; ARCH=${ARCH:-gfx950}
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
SRCS=$(sed -n 's/^HIP_SRCS *:= *//p' "$B/aliparaformerasr_amd/csrc/Makefile")
mkflags() { sed -n 's/^CXXFLAGS *:= *//p' "$1/aliparaformerasr_amd/csrc/Makefile" | sed "s/\$(ARCH)/$ARCH/; s/\$(EXTRA)/${EXTRA:-}/"; }
for side in A B; do
  tree=${!side}; mkdir -p "$TMP/$side"
  for f in $SRCS; do
    [ -f "$tree/aliparaformerasr_amd/csrc/$f" ] || { : > "$TMP/$side/${f%.hip}.s"; continue; }   # a source only the other tree has
    ( fl="$(mkflags "$tree") -w"; [ "$f" = k_pcm.hip ] && fl="$fl -ffp-contract=off"
      cd "$tree/aliparaformerasr_amd/csrc" && "$HIPCC" $fl --offload-device-only -S "$f" -o - |
        grep -vE '^\s*(;|\.ident|\.file|\.loc|\.cfi_|\.section\s+\.debug)' | sed -E 's/\s*;.*$//' > "$TMP/$side/${f%.hip}.s" ) &
    while [ "$(jobs -rp | wc -l)" -ge "${JOBS:-16}" ]; do wait -n; done
  done
done
wait
python3 - "$TMP" $SRCS > "$OUT" <<'EOF'
import json, re, sys
tmp, srcs = sys.argv[1], sys.argv[2:]
def kernels(path):                      # name -> resources (from the .amdhsa metadata) + instruction lines of its body
    text, out = open(path).read(), {}
    for m in re.finditer(r"^(\w+):\n(.*?)^\.Lfunc_end", text, re.M | re.S):
        out[m.group(1)] = {"instructions": sum(1 for l in m.group(2).splitlines() if re.match(r"\s+[a-z]\w+", l) and not l.lstrip().startswith(".")),
                           "_text": m.group(2).replace(m.group(1), "K")}
    for m in re.finditer(r"\.amdhsa_kernel (\w+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        if m.group(1) in out:
            out[m.group(1)]["_text"] += m.group(2)
    for m in re.finditer(r"\.name:\s+(\w+)\n(.*?)(?=\n\s+- \.|\namdhsa\.|\Z)", text, re.S):
        if m.group(1) in out:
            for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size"):
                v = re.search(r"\." + key + r":\s+(\d+)", m.group(2))
                if v: out[m.group(1)][key] = int(v.group(1))
    return out
res = {}
for f in srcs:
    a, b = (f"{tmp}/{s}/{f[:-4]}.s" for s in "AB")
    ka, kb = kernels(a), kernels(b)
    res[f] = {"identical": open(a).read() == open(b).read() and len(open(a).read()) > 0, "a": ka, "b": kb}
    if not res[f]["identical"]:
        res[f]["a_kernels_in_b"] = {n: next((m for m, y in kb.items() if y["_text"] == x["_text"]), None) for n, x in ka.items()}
    for k in list(ka.values()) + list(kb.values()):
        del k["_text"]
json.dump(res, sys.stdout, indent=1, sort_keys=True)
print()
print("\n".join(f"{f}: {'identical' if r['identical'] else 'DIFFERENT'}" for f, r in res.items()), file=sys.stderr)
for f, r in res.items():
    for n, m in r.get("a_kernels_in_b", {}).items():
        print(f"  {f}: {n[:60]} -> {'the same code as ' + m[:60] if m else 'NO kernel of B has this code'}", file=sys.stderr)
EOF
