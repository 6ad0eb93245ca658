"""Summarise `hipcc -Rpass-analysis=kernel-resource-usage` output (stderr log) per kernel.

    resusage.py LOG                 one line per kernel, short names (sweep_kernel decoded, others cut at 40 characters)
    resusage.py --full LOG [LOG..]  one line per kernel keyed by the full mangled name, sorted, all figures: two builds have the same device
                                    code interface when `diff` of the two outputs is empty (same kernels, same registers / scratch / LDS)
"""
import re
import sys

KEYS = [('vgpr', 'VGPRs'), ('agpr', 'AGPRs'), ('sgpr', 'SGPRs'), ('scratch', 'ScratchSize [bytes/lane]'), ('occ', 'Occupancy [waves/SIMD]'),
        ('vspill', 'VGPRs Spill'), ('sspill', 'SGPRs Spill'), ('lds', 'LDS Size [bytes/block]')]


def kernels(path):
    for b in open(path).read().split('Function Name: ')[1:]:
        def g(k):
            m = re.search(re.escape(k) + r': (\d+)', b)
            return int(m.group(1)) if m else -1
        yield b.split()[0], {short: g(key) for short, key in KEYS}


full = len(sys.argv) > 1 and sys.argv[1] == '--full'
if full:
    lines = []
    for path in sys.argv[2:]:
        for name, v in kernels(path):
            lines.append(name + ' ' + ' '.join('%s=%d' % (k, v[k]) for k, _ in KEYS))
    print('\n'.join(sorted(lines)))
else:
    for name, v in kernels(sys.argv[1]):
        m = re.search(r'sweep_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E', name)
        short = "sweep<G=%s,R=%s,W=%s,L=%s>" % m.groups() if m else name[:40]
        print("%-34s vgpr=%d agpr=%d sgpr=%d scratch=%d occ=%d vspill=%d lds=%d" % (
            short, v['vgpr'], v['agpr'], v['sgpr'], v['scratch'], v['occ'], v['vspill'], v['lds']))
