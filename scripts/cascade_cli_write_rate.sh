#!/bin/bash
# CLI end to end, write sink behind a cascade: the fused plan (k_cascade_write for the full 0x1000-sample blocks) vs the block
# iterator (QUADRS_HIP_NO_FUSE=1) on one 1 GiB cf32 file, output files compared byte for byte, for a shift-free chain (LL) and the
# bench chain with its shift (SLL).  usage: scripts/cascade_cli_write_rate.sh [out dir, default build/cascade_cli_write]
out=${1:-build/cascade_cli_write}
mkdir -p $out
f=${TMPDIR:-/tmp}/cascade-write-rate.sr21M.cf32
python3 -c "
import numpy as np
n, piece = (1 << 30) // 8, 1 << 24
rng = np.random.default_rng(1)
with open('$f', 'wb') as fh:
    for a in range(0, n, piece):
        t = np.arange(a, a + piece)
        z = 0.2 * np.exp(2j * np.pi * 0.0133 * t) + 0.01 * rng.standard_normal(piece)
        np.stack([z.real, z.imag], 1).astype(np.float32).tofile(fh)"
cli=quadrs_amd/quadrs-hip
lp="lowpass -decimate 4 2000000 lowpass -power 100 -decimate 8 200000"
for leg in LL SLL; do
    if [ $leg = LL ]; then chain="from $f $lp"; else chain="from $f shift 280000 $lp"; fi
    rm -f $out/$leg-*.sr*.cf32
    $cli $chain write $out/$leg-warm > /dev/null 2>&1                 # first touch: page cache, device init
    t0=$(date +%s.%N); $cli $chain write $out/$leg-fused; rc1=$?; t1=$(date +%s.%N)
    QUADRS_HIP_NO_FUSE=1 timeout 1500 $cli $chain write $out/$leg-iter; rc2=$?; t2=$(date +%s.%N)
    python3 -c "
import glob, hashlib, json
import numpy as np
a = open(glob.glob('$out/$leg-fused.sr*.cf32')[0], 'rb').read()
b = open(glob.glob('$out/$leg-iter.sr*.cf32')[0], 'rb').read()
fused, it = $t1 - $t0, $t2 - $t1
x, y = np.frombuffer(a, np.uint32), np.frombuffer(b, np.uint32)
diff = int((x != y).sum()) if x.size == y.size else -1
print(json.dumps({'leg': '$leg', 'file_bytes': 1 << 30, 'chain': '$chain write OUT'.replace('$f', 'FILE.sr21M.cf32'), 'fused_s': fused,
                  'fused_rc': $rc1, 'iterator_s': it, 'iterator_rc': $rc2, 'speedup': it / fused, 'out_bytes': len(a),
                  'identical': a == b, 'differing_words': diff, 'sha256': hashlib.sha256(a).hexdigest()}, indent=1))" | tee $out/$leg.json
    rm -f $out/$leg-*.sr*.cf32
done
rm -f $f
