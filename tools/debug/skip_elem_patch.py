# TEMPORARY timing experiment, never committed applied: rewrites elem.hip / dense.hip / gemm.hip so that the bit mask in
# CMOOP_DEBUG_SKIP_ELEM drops whole kernel families (results are garbage, only the wall time means something):
#   1 BatchNorm (statistics finalize, apply, fused pool forms, backward reduce / apply)   2 first conv (C_in = 1) fwd / wgrad
#   4 dense head + GAP + softmax-CE (softmax_ce_kernel<...>: all three training losses)
#                                                                                          8 max-pool, add+ReLU
#  16 Adam (with the slab sums), step state                                               32 split-K combine + flip-transpose
# Apply, make, run tools/debug/skip_run.sh on the GPU, then `git checkout` the three files and rebuild.
import re
root = '/root/repo/cmoop_audio_processing_amd/csrc/'
FAMILY = [(1, r'colreduce_kernel|bn_\w+|scale_shift_kernel'), (2, r'conv1_\w+'),
          (4, r'dense_\w+|gap_\w+|softmax_ce_kernel|colsum_\w+|confusion_kernel'), (8, r'maxpool_\w+|add_relu_kernel'),
          (16, r'adam_\w+|step_advance_kernel'),   # NOT the shuffle / init kernels: skipping epoch_permutation_kernel left the first conv's
          # gather indices undefined and faulted the GPU in round 2 (profiles/r02_non_gemm_cost_upper_bound.txt); the gather is clamped since round 3
          (32, r'splitk_combine_kernel|flip_transpose_all_kernel')]
hdr = '''
#include <cstdlib>
static inline int dbg_skip_mask() { static const int v = getenv("CMOOP_DEBUG_SKIP_ELEM") ? atoi(getenv("CMOOP_DEBUG_SKIP_ELEM")) : 0; return v; }
#define ELEM_LAUNCH(MASK, ...) do { if (!(dbg_skip_mask() & (MASK))) hipLaunchKernelGGL(__VA_ARGS__); } while (0)
'''
def family(name):
    for bit, rx in FAMILY:
        if re.fullmatch(rx, name): return bit
    return None
for f in ('elem.hip', 'dense.hip', 'gemm.hip'):
    s = open(root + f).read()
    def sub(m):
        bit = family(m.group(2))
        return m.group(0) if bit is None else f'ELEM_LAUNCH({bit}, {m.group(1)}{m.group(2)}'
    s, n = re.subn(r'hipLaunchKernelGGL\((\(?)([A-Za-z_0-9]+)', sub, s)
    idx = [m.end() for m in re.finditer(r'^#include.*$', s, re.M)][-1]
    open(root + f, 'w').write(s[:idx] + hdr + s[idx:])
    print(f, s.count('ELEM_LAUNCH('))
