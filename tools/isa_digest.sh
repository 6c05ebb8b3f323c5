#!/bin/bash
# Per-kernel instruction digest of a built object: bash tools/isa_digest.sh <obj.o> <out.txt>
# Unbundles the gfx950 code object (as tools/kres.sh does), disassembles it and writes one line per
# function symbol:  <sha1 of its instruction text> <instruction count> <sha1 of its sorted mnemonic
# histogram> <symbol>,  sorted by symbol.  Two builds whose lines agree run the same instructions; lines
# that agree in all but the first column differ only in operands (register naming, local order).
#   bash tools/isa_digest.sh --compare <a.txt> <b.txt>   lists, per symbol, identical / same-histogram /
#   different / only in one, and the totals.
set -e
if [ "$1" = "--compare" ]; then
  exec python3 - "$2" "$3" <<'EOF'
import sys
def load(p):
    d = {}
    for line in open(p):
        h, n, m, sym = line.split(None, 3)
        d[sym.strip()] = (h, n, m)
    return d
a, b = load(sys.argv[1]), load(sys.argv[2])
same = hist = diff = 0
for s in sorted(set(a) | set(b)):
    if s not in a or s not in b:
        print("only in", sys.argv[1] if s in a else sys.argv[2], s)
    elif a[s] == b[s]:
        same += 1
    elif a[s][1:] == b[s][1:]:
        hist += 1
        print("same count and histogram, text differs:", a[s][1], s)
    else:
        diff += 1
        print("different:", a[s][1], "->", b[s][1], s)
print(f"{len(a)} symbols vs {len(b)}: {same} identical, {hist} same count and histogram, {diff} different, "
      f"{len(set(a) - set(b))} only in the first, {len(set(b) - set(a))} only in the second")
EOF
fi
T=$(mktemp -d)
/opt/rocm/lib/llvm/bin/llvm-objcopy --dump-section=.hip_fatbin=$T/fb "$1"
/opt/rocm/lib/llvm/bin/clang-offload-bundler --type=o --input=$T/fb --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/dev.o --unbundle
/opt/rocm/lib/llvm/bin/llvm-objdump -d --no-show-raw-insn --no-leading-addr $T/dev.o | python3 -c "
import sys, re, hashlib, collections
sym, text = None, {}
for line in sys.stdin:
    m = re.match(r'^[0-9a-f]* ?<(.+)>:\s*$', line)
    if m:
        sym = m.group(1)
        text[sym] = []
    elif sym and line.strip():  # (this objdump still appends '// address: encoding' to every line: dropped)
        text[sym].append(line.split('//')[0].strip())
for s in sorted(text):
    ins = text[s]
    hist = collections.Counter(i.split()[0] for i in ins)
    h = hashlib.sha1('\n'.join(ins).encode()).hexdigest()
    hh = hashlib.sha1('\n'.join(f'{k} {v}' for k, v in sorted(hist.items())).encode()).hexdigest()
    print(h, len(ins), hh, s)
" > "$2"
rm -rf $T
