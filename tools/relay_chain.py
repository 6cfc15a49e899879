"""The relay-token block per H-OSA iteration, from a rocprofv3 --kernel-trace CSV of bench.py: first kernel's start to last
kernel's end of the block's launches.  Five-launch path: ln_qkv_fused -> relay_attn_f16 -> gemm_x3 (proj) -> ln_mlp_fused ->
mlp_tail_reduce on one queue, found around every relay_attn_f16_kernel; one-launch path: every relay_block_fused_kernel.
Prints the per-kernel medians and the median / quartiles of the chain over the last 30 instances (10 iterations of the last
three forwards).
    python tools/relay_chain.py <kernel_trace.csv> [instances, default 30]"""
import csv
import statistics
import sys


def quart(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[0], q[2]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    keep = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    byq = {}
    for r in rows:
        byq.setdefault(r['Queue_Id'], []).append(r)
    chains = []
    for q in byq.values():
        for i, r in enumerate(q):
            n = r['Kernel_Name']
            if 'relay_block_fused_kernel' in n:
                chains.append([r])
            elif 'relay_attn_f16_kernel' in n and i >= 1 and i + 3 < len(q):
                c = q[i - 1:i + 4]
                want = ('ln_qkv_fused', 'relay_attn_f16', 'gemm_x3', 'ln_mlp_fused', 'mlp_tail_reduce')
                if all(w in k['Kernel_Name'] for w, k in zip(want, c)):
                    chains.append(c)
                else:
                    print('unexpected neighbours of relay_attn_f16_kernel:', [k['Kernel_Name'][:60] for k in c], file=sys.stderr)
    chains.sort(key=lambda c: int(c[0]['Start_Timestamp']))
    chains = chains[-keep:]
    if not chains:
        raise SystemExit('no relay-token block in the trace')
    span = [(int(c[-1]['End_Timestamp']) - int(c[0]['Start_Timestamp'])) / 1e3 for c in chains]
    print('%d instances, %d launches each' % (len(chains), len(chains[0])))
    for j in range(len(chains[0])):
        d = [(int(c[j]['End_Timestamp']) - int(c[j]['Start_Timestamp'])) / 1e3 for c in chains]
        print('  %-44s median %6.1f us  grid %s wg %s' % (chains[0][j]['Kernel_Name'].split('(anonymous namespace)::')[-1][:44],
                                                        statistics.median(d), chains[0][j].get('Grid_Size_X', '?'),
                                                        chains[0][j].get('Workgroup_Size_X', '?')))
    m, q1, q3 = quart(span)
    print('chain start-to-end: median %.1f us  quartiles %.1f .. %.1f (IQR %.1f)  min %.1f max %.1f'
          % (m, q1, q3, q3 - q1, min(span), max(span)))


if __name__ == '__main__':
    main()
