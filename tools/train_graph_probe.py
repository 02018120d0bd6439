"""Developer probe (GPU box): phases of the recorded (hipGraph) full-size training step."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tf_flowavenet_amd.hparams import default_hparams
from tf_flowavenet_amd import weights as W, training as TR

hp = default_hparams()
b, t = 8, 6400
inp = W.synthetic_inputs(hp, b, t)
x, c = torch.from_numpy(inp["x"]).reshape(b, t).cuda(), torch.from_numpy(inp["c"]).cuda()
tr = TR.Trainer(hp, W.synthetic_params(hp, 1234), graph=True)
tr.ddi(x, c)
for _ in range(3):
    tr.step(x, c)
torch.cuda.synchronize()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10
t00 = time.perf_counter()
for _ in range(n):
    tr.opt.advance()
    for g, i in tr._recorded[next(iter(tr._recorded))]["segs"]:
        if g is not None:
            g.replay()
    torch.cuda.synchronize()
print("per step: replay + drain %.2f ms" % ((time.perf_counter() - t00) / n * 1e3))
