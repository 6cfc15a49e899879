"""The pooling head of EVERY complete forward in a rocprofv3 --kernel-trace CSV of the bench step (tools/forward_phases.py looks
at the last one only): wall from the first attn_pool_kernel to the forward's last kernel end, launches, and busy time per
kernel, so that a change of the phase can be set against its spread over the forwards of one run.
    python tools/pooling_head_spread.py <kernel_trace.csv>"""
import collections, csv, re, sys
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
starts, last = [], -10 ** 18
for i, r in enumerate(rows):
    if 'tap_count_kernel' in r['Kernel_Name']:
        t = int(r['Start_Timestamp'])
        if t - last > 1000000:
            starts.append(i)
        last = t
walls, counts, per = [], [], collections.defaultdict(list)
for a, b in zip(starts[:-1], starts[1:]):
    fwd = rows[a:b]
    th = next((int(r['Start_Timestamp']) for r in fwd if 'attn_pool_kernel' in r['Kernel_Name']), None)
    if th is None:
        continue
    head = [r for r in fwd if int(r['Start_Timestamp']) >= th]
    walls.append((max(int(r['End_Timestamp']) for r in head) - th) / 1e3)
    counts.append(len(head))
    tot = collections.Counter(); n = collections.Counter()
    for r in head:
        k = re.sub(r'\(.*', '', r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', ''))[:70]
        tot[k] += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3; n[k] += 1
    for k in tot:
        per[k].append((n[k], tot[k]))
walls_s = sorted(walls)
print('pooling head over %d forwards: wall us min %.1f median %.1f max %.1f (all: %s); launches %s'
      % (len(walls), walls_s[0], walls_s[len(walls_s) // 2], walls_s[-1], ' '.join('%.1f' % w for w in walls), sorted(set(counts))))
for k, v in sorted(per.items(), key=lambda kv: -sum(t for _, t in kv[1])):
    print('  %-70s x%d  %.1f us per forward' % (k, v[0][0], sum(t for _, t in v) / len(v)))
