"""tests/_cpu_feeder.py's stand-in with the NDC methods of HipFeeder (TEST INFRASTRUCTURE: the product has no CPU path): the
same float32 torch rays, taken through the host formula plenoctree_amd.nerf_sh.nerf.llff.convert_to_ndc.  The viewdirs
stay the world-space unit directions, as in the reference (nerf_sh/nerf/datasets.py:337-345).  tests/test_llff_cpu.py
installs it on the LLFF class for datasets built on a CPU device."""
from _cpu_feeder import CpuFeeder
from plenoctree_amd.nerf_sh.nerf import llff


class LlffCpuFeeder(CpuFeeder):
    def generate_rays_ndc(self, c2w, w, h, focal, ray_indices, ndc_near=1.0):
        o, d, v = self.generate_rays(c2w, w, h, focal, ray_indices)
        o, d = llff.convert_to_ndc(o, d, focal, w, h, near=ndc_near)
        return o.contiguous(), d.contiguous(), v

    def generate_rays_multi_ndc(self, c2w_all, w, h, focal, ray_ids, ndc_near=1.0):
        o, d, v = self.generate_rays_multi(c2w_all, w, h, focal, ray_ids)
        o, d = llff.convert_to_ndc(o, d, focal, w, h, near=ndc_near)
        return o.contiguous(), d.contiguous(), v


def feeder_for(device):
    """HipFeeder on a ROCm device, LlffCpuFeeder on the CPU (tests only)."""
    if device.type == "cuda":
        from plenoctree_amd.nerf_sh.nerf.datasets import HipFeeder
        return HipFeeder(device)
    return LlffCpuFeeder(device)
