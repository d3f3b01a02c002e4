"""What the category-prediction loss costs a training step: CROWN-CROWN ``TrainStep.step`` at the train2b shape (batch 32, K = 1 + 4,
history 50, title 32 + body 128, fp32, dropout off) with ``alpha = 0`` and ``alpha = 0.3``, alternated in one process after a warm-up.

``alpha = 0`` stands for the code before the loss existed: it is that code path -- the tool asserts that the attribute stays None and
that the bucket holds no ``category_predictor`` parameter.  ``alpha = 0.3`` adds lime_linear_xent_f32 on the B H history rows,
the row sum, the classifier's weight gradient and two scalings to every step.

The bare CROWN-CROWN model refines a 900-wide history: the candidate-aware attention's training kernel (cand_attn_train_kernel) holds
a row's N + H topic projections and its per-head weights in LDS and takes H <= 33 at that width, so the train2b history of 50 is refused
with its status before any launch (a limit of the kernel, not of the loss).  ``--history`` sets the history length; the recorded run
is ``--history 32``, B H = 1,024 history rows.

Per arm and round: the median of ``--steps`` device-event step times; reported: the median over ``--rounds`` rounds with min ... max.
Prints one JSON line and writes it to ``--json-out`` (default profiles/aux_loss.json).

    python tools/bench_aux_loss.py --rounds 3 --history 32
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from lime_cikm25_amd import Model, make_config, synth  # noqa: E402
from lime_cikm25_amd.training import TrainStep  # noqa: E402

ARMS = (0.0, 0.3)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--candidates', type=int, default=5)
    ap.add_argument('--history', type=int, default=None, help='max_history_num (default: the configuration\'s 50)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--json-out', default=os.path.join(ROOT, 'profiles', 'aux_loss.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_aux_loss.py measures on the GPU: there is no CPU path'

    steps, batch = {}, None
    for alpha in ARMS:
        cfg = make_config(news_encoder='CROWN', user_encoder='CROWN', alpha=alpha,
                          **({} if args.history is None else dict(max_history_num=args.history)))
        torch.manual_seed(0)
        model = Model(cfg)
        model.initialize()
        synth.fill_state_dict(model, seed=args.seed)
        model = model.cuda().eval()
        model.training = True                                              # the differentiable path with every child in eval mode
        step = TrainStep(model, lr=1e-4, gradient_clip_norm=4.0)
        fc = [n for n in step.names if 'category_predictor.' in n]
        assert len(fc) == (2 if alpha else 0), fc
        steps[alpha] = step
        if batch is None:
            batch = [v.cuda() for v in synth.make_batch(cfg, args.batch, args.candidates, seed=args.seed).values()]

    def one(alpha):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = steps[alpha].step(*batch)
        e1.record()
        e1.synchronize()
        aux = steps[alpha].model.news_encoder.auxiliary_loss
        assert (aux is None) == (alpha == 0.0), 'alpha = %s: auxiliary_loss %r' % (alpha, aux)
        return e0.elapsed_time(e1), float(loss), (None if aux is None else float(aux))

    for _ in range(args.warmup):
        for alpha in ARMS:
            one(alpha)
    torch.cuda.synchronize()
    medians, last = {a: [] for a in ARMS}, {}
    for r in range(args.rounds):
        for alpha in ARMS:
            ms = []
            for _ in range(args.steps):
                dt, loss, aux = one(alpha)
                ms.append(dt)
            medians[alpha].append(statistics.median(ms))
            last[alpha] = (loss, aux)
            say('round %d alpha %.1f: median %.3f ms (min %.3f, max %.3f) loss %.5f aux %s' % (r, alpha, medians[alpha][-1], min(ms), max(ms),
                                                                                         loss, aux))
    stat = lambda v: {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    off, on = stat(medians[0.0]), stat(medians[0.3])
    H = steps[0.0].model.config.max_history_num
    line = dict(bench='aux_loss', model='CROWN-CROWN', shape='train2b', batch=args.batch, candidates=args.candidates,
                history=H, history_rows=args.batch * H, rounds=args.rounds, steps_per_round=args.steps,
                alpha_0_step_ms=off, alpha_03_step_ms=on, on_over_off=round(on['median'] / off['median'], 4),
                added_ms=round(on['median'] - off['median'], 3), last_loss_alpha_0=last[0.0][0], last_loss_alpha_03=last[0.3][0],
                last_aux_alpha_03=last[0.3][1], device=torch.cuda.get_device_name(0))
    print(json.dumps(line))
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, 'w') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
