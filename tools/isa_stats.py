"""Head / tail figures of a kernel from hipcc's device assembly (the evidence file profiles/expert_gemm_plain_isa.txt).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S tutel_amd/csrc/expert_gemm.hip -o expert_gemm.s
    python tools/isa_stats.py expert_gemm.s 'expert_gemm_big_kernelI6__bf16Lb1ELi1ELi4ELi3ELb1ELi128ELb1E'

Counts are in text order over the kernel's body (labels, directives and comments left out):
  head = the instructions in front of the first LDS-DMA (a buffer / global load with the `lds` modifier): how many, the scalar loads
         among them, the s_waitcnt that name lgkmcnt and those that name vmcnt, the expansions of an integer division by a run-time
         divisor (one v_rcp_iflag_f32 each);
  tail = the instructions behind the last MFMA: how many, the loads (scalar, global, buffer; LDS reads are not loads from memory) and
         the division expansions; plus whether any global / buffer load that is not an LDS-DMA stands in front of the last MFMA;
  resources as hipcc prints them behind the kernel.
"""
import re
import sys


def kernels(path):
    """name -> (instructions of the body in text order, resource figures hipcc prints behind the body)"""
    out, name, body, res = {}, None, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body, res = m.group(1), [], {}
            out[name] = (body, res)
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            body = None
            continue
        if body is not None:
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                body.append(s)
        else:
            m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|LDSByteSize|Occupancy): (\d+)", line)
            if m:
                res.setdefault(m.group(1), int(m.group(2)))
    return out


def stats(body):
    op = [s.split()[0] for s in body]
    is_dma = [bool(re.match(r"(buffer|global)_load_", s)) and bool(re.search(r"\blds\b", s)) for s in body]
    first_dma = is_dma.index(True) if True in is_dma else len(body)
    mf = [i for i, o in enumerate(op) if o.startswith("v_mfma")]
    last_mfma = mf[-1] if mf else -1
    head, tail = body[:first_dma], body[last_mfma + 1:]
    div = lambda part: sum(s.startswith("v_rcp_iflag_f32") for s in part)
    mem_load = lambda s, dma: bool(re.match(r"(s_load|s_buffer_load|global_load|buffer_load|flat_load|scratch_load)", s)) and not dma
    return dict(
        total=len(body), head=first_dma,
        head_s_loads=sum(s.startswith(("s_load", "s_buffer_load")) for s in head),
        head_lgkm_waits=sum(s.startswith("s_waitcnt") and "lgkmcnt" in s for s in head),
        head_vm_waits=sum(s.startswith("s_waitcnt") and "vmcnt" in s for s in head),
        head_div=div(head), tail=len(tail), tail_loads=sum(mem_load(s, False) for s in tail), tail_div=div(tail), div_total=div(body),
        vector_loads_before_last_mfma=sum(mem_load(s, d) and not s.startswith("s_") for s, d in zip(body[:last_mfma + 1], is_dma[:last_mfma + 1])),
    )


def main():
    path, pats = sys.argv[1], sys.argv[2:]
    for name, (body, res) in kernels(path).items():
        if pats and not any(p in name for p in pats):
            continue
        st = stats(body)
        print(name)
        print("  instructions %(total)d | ahead of the first LDS-DMA: %(head)d instructions, %(head_s_loads)d scalar loads, %(head_lgkm_waits)d lgkmcnt waits, "
              "%(head_vm_waits)d vmcnt waits, %(head_div)d division expansions" % st)
        print("  after the last MFMA: %(tail)d instructions, %(tail_loads)d loads, %(tail_div)d division expansions | division expansions in all: %(div_total)d | "
              "vector loads (not LDS-DMA) ahead of the last MFMA: %(vector_loads_before_last_mfma)d" % st)
        print("  resources (LDS is dynamic: see the plan's lds_bytes): " + ", ".join("%s %d" % kv for kv in res.items()))


if __name__ == "__main__":
    main()
