"""What the DecodeRunner tests share (test_paged_prefill_runner_gpu, test_verify_runner_gpu, test_verify_tree_runner_gpu,
test_sampling_runner_gpu): one runner shape -- LlamaConfig.tiny, B = 3, pools for 70 + 100 tokens, eager launches, fusion level
2 --, one prompt of L = 150 tokens per sequence, drafts of N = 4 positions, and the state and distance helpers around them."""
import torch

B, L, N = 3, 150, 4


def runner(sampling=False, use_graph=False, seed=11):
    from omniserve_amd.runtime import DecodeRunner, LlamaConfig
    return DecodeRunner(LlamaConfig.tiny(), B, 70, 100, torch.device("cuda:0"), seed=seed, use_graph=use_graph, fused=2,
                        sampling=sampling)


def prompt(r, n=L):
    g = torch.Generator(device=r.device)
    g.manual_seed(5)
    return torch.randint(0, r.cfg.vocab, (B, n), device=r.device, generator=g)


def prefilled(sampling=False, use_graph=False, **params):
    """A runner behind prefill(L, the prompt), set_sampling(**params) first where given.  -> (runner, (lengths, tokens))."""
    r = runner(sampling, use_graph)
    if params:
        r.set_sampling(**params)
    r.prefill(L, prompt(r).reshape(-1))
    return r, (r.lengths.clone(), r.tokens.clone())


def restore(r, state):
    r.lengths.copy_(state[0])
    r.tokens.copy_(state[1])


def random_draft(r, seed, n=N):
    g = torch.Generator(device=r.device)
    g.manual_seed(seed)
    tail = torch.randint(0, r.cfg.vocab, (B, n - 1), device=r.device, generator=g)
    return torch.cat([r.tokens.view(B, 1), tail], dim=1)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).norm(dim=-1) / b.norm(dim=-1)).max())


def pools(r):
    return [[p.clone() for p in layer] for layer in r.pools]


def four_steps(r):
    toks = []
    for _ in range(4):
        r.step()
        toks.append(r.tokens.clone())
    torch.cuda.synchronize()
    return torch.stack(toks), r.x.clone()
