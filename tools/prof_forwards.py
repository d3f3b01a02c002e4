"""The forwards of a rocprofv3 (rocpd sqlite) kernel trace of ``bench.py --plain`` with the branches forked on side streams, where the
launches of two forwards need not start in the same order and ``prof_summary.py --timeline`` finds no period: a forward is what lies
between two ``multi_copy_kernel`` launches (the input staging in front of every graph replay).  Prints the medians over the later three
quarters of the trace -- head (first kernel -> start of the body's ``token_attn_sp_vocab_kernel<4>``), tail (end of the last
``ffn_sp_kernel`` -> end of the forward), wall, kernel-busy, ``batch_scan_kernel`` -- and the middle forward with real start and end times.

    python tools/prof_forwards.py /tmp/prof/p_results.db
"""
import sqlite3
import sys


def main():
    c = sqlite3.connect(sys.argv[1])
    short = lambda n: n.replace('(anonymous namespace)::', '').replace('void ', '')
    rows = [(short(n), s, e) for n, s, e in c.execute('select name, start, end from kernels order by start').fetchall()]
    marks = [i for i, r in enumerate(rows) if r[0].startswith('multi_copy_kernel')]
    fw = []
    for a, b in zip(marks[:-1], marks[1:]):
        seq = rows[a:b]
        while seq and seq[-1][0].startswith('__amd_rocclr_copyBuffer'):      # (the copy in front of multi_copy belongs to the next forward)
            seq = seq[:-1]
        fw.append(seq)
    lens = sorted(len(s) for s in fw)
    print('forwards: %d, launches per forward (median, without the host copy in front): %d' % (len(fw), lens[len(lens) // 2]))
    stats = []
    for seq in fw[len(fw) // 4:]:
        t0 = seq[0][1]
        att = [s for n, s, e in seq if n.startswith('token_attn_sp_vocab_kernel<4>')]
        ffn = [e for n, s, e in seq if n.startswith('ffn_sp_kernel')]
        if not att or not ffn:
            continue
        end = max(e for n, s, e in seq)
        scan = [e - s for n, s, e in seq if n.startswith('batch_scan_kernel')]
        stats.append(((att[0] - t0) / 1e3, (end - max(ffn)) / 1e3, (end - t0) / 1e3, sum(e - s for n, s, e in seq) / 1e3,
                      scan[0] / 1e3 if scan else 0.0))
    if stats:
        med = lambda k: sorted(x[k] for x in stats)[len(stats) // 2]
        print('median over %d forwards: head %.1f us, tail %.1f us, wall %.1f us, kernel-busy %.1f us, batch_scan %.1f us'
              % (len(stats), med(0), med(1), med(2), med(3), med(4)))
    seq = fw[len(fw) // 2]
    t0 = seq[0][1]
    for n, s, e in seq:
        print('%9.1f us  +%8.1f us  (end %9.1f)  %s' % ((s - t0) / 1e3, (e - s) / 1e3, (e - t0) / 1e3, n[:100]))


if __name__ == '__main__':
    main()
