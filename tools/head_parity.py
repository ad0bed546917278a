"""The field head against its binary64 model: the share of each running bound the kernels use, per output and per block of
head_cases' rows, and the same figures for the model evaluated with binary32 operations on the CPU.

    python tools/head_parity.py [--out profiles/head_parity.json]

It makes the calls tests/test_head_gpu.py makes (its own helpers) and asserts nothing: the tests do.  Needs a GPU."""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "make-it-3d_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import head_model as H  # noqa: E402
import test_head_gpu as T  # noqa: E402


def _merge(worst, fig):
    for k, v in fig.items():
        if k == "blocks":
            for b, d in v.items():
                for name, val in d.items():
                    worst["blocks"].setdefault(b, {})[name] = max(worst["blocks"].get(b, {}).get(name, 0.0), val)
        else:
            worst[k] = max(worst.get(k, 0.0), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_parity.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cuda = torch.device("cuda:0")
    entries, failed = [], []
    cpu, gpu_f, gpu_b = {"blocks": {}}, {"blocks": {}}, {"blocks": {}}
    for P in (7, 13):
        for i, params in enumerate(H.PARAMS):
            case, dev = T.head_case(P, 4099, i, cuda)
            fig, fails = H.check(H.as_got(H.model_of(case, acc=torch.float32)), H.model_of(case), case["blocks"])
            entries.append(dict(case="cpu_binary32_model", P=P, n=4099, params=list(params), failed=fails, **fig))
            _merge(cpu, fig)
            for n in T.SIZES:
                case, dev = T.head_case(P, n, i, cuda)
                _, (fig, fails) = T.forward_figures(case, dev)
                entries.append(dict(case="forward", P=P, n=n, params=list(params), failed=fails, **fig))
                _merge(gpu_f, fig)
                failed += fails
            case, dev = T.head_case(P, 4099, i, cuda)
            for P_active in (1, 7, 13):
                if P_active > P:
                    continue
                names = T.ALLOWED[P_active]
                for k in range(len(names) + 1):
                    for grads in itertools.combinations(names, k):
                        _, (fig, fails) = T.backward_figures(case, dev, P_active, grads)
                        entries.append(dict(case="backward", P=P, P_active=P_active, n=4099, params=list(params),
                                            grads=list(grads), failed=fails, **fig))
                        _merge(gpu_b, fig)
                        failed += fails
    report = dict(device=torch.cuda.get_device_name(0), worst_cpu_binary32_model=cpu, worst_forward=gpu_f,
                  worst_backward=gpu_b, failed=sorted(set(failed)), cases=entries)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=0)
    for name in ("worst_cpu_binary32_model", "worst_forward", "worst_backward"):
        print(f"[head] {name}: {H.worst(report[name])}")
    print(f"[head] failed assertions: {report['failed'] or 'none'} -> {args.out}")


if __name__ == "__main__":
    main()
