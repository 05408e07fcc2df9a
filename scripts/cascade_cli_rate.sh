#!/bin/bash
# CLI end to end on a cascaded chain: the fused cascade plan vs the block iterator (QUADRS_HIP_NO_FUSE=1) on one 256 MiB cf32
# file, stdout compared byte for byte.  usage: scripts/cascade_cli_rate.sh [out dir, default build/cascade_cli]
out=${1:-build/cascade_cli}
mkdir -p $out
f=${TMPDIR:-/tmp}/cascade-rate.sr21M.cf32
python3 -c "
import numpy as np
n = (256 << 20) // 8
t = np.arange(n)
z = 0.2 * np.exp(2j * np.pi * 0.0133 * t) + 0.01 * np.random.default_rng(1).standard_normal(n)
np.stack([z.real, z.imag], 1).astype(np.float32).tofile('$f')"
chain="from $f shift 280000 lowpass -decimate 4 2000000 lowpass -power 100 -decimate 8 200000 sparkfft -width 128"
cli=quadrs_amd/quadrs-hip
$cli $chain > /dev/null                                     # first touch: page cache, device init
t0=$(date +%s.%N); $cli $chain > $out/fused.txt; rc1=$?; t1=$(date +%s.%N)
QUADRS_HIP_NO_FUSE=1 timeout 1500 $cli $chain > $out/iter.txt; rc2=$?; t2=$(date +%s.%N)
python3 -c "
import json, hashlib
a, b = open('$out/fused.txt', 'rb').read(), open('$out/iter.txt', 'rb').read()
fused, it = $t1 - $t0, $t2 - $t1
print(json.dumps({'file_bytes': 256 << 20, 'chain': '$chain'.replace('$f', 'FILE.sr21M.cf32'), 'fused_s': fused, 'fused_rc': $rc1,
                  'iterator_s': it, 'iterator_rc': $rc2, 'speedup': it / fused, 'rows': a.count(b'\n') - 1,
                  'stdout_identical': a == b, 'stdout_sha256': hashlib.sha256(a).hexdigest()}, indent=1))" | tee $out/cascade_cli.json
rm -f $f $out/iter.txt
