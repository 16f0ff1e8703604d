"""Shared by the GPU tests of the fused dense-block kernel (test_gpu_rdb_*.py): an RRDBNet with the fused path forced
on or off, and the launch count of one forward."""
import os

import torch


def net(sd, num_block, fuse, num_in_ch=3, scale=2):
    """RRDBNet on cuda:0 with NESR_RDB_FUSE = -1 (fuse) or 0 in force while its context is created; the environment is restored."""
    from neural_enhanced_super_resolution_amd import RRDBNet
    old = os.environ.get("NESR_RDB_FUSE")
    os.environ["NESR_RDB_FUSE"] = "-1" if fuse else "0"
    try:
        n = RRDBNet(num_in_ch, 3, scale=scale, num_block=num_block)
        n.load_state_dict(sd)
        n.eval().to("cuda:0")
        n(torch.zeros(1, num_in_ch, 16, 16, device="cuda:0"))        # the context is created with the switch in force
    finally:
        if old is None:
            os.environ.pop("NESR_RDB_FUSE", None)
        else:
            os.environ["NESR_RDB_FUSE"] = old
    return n


def launches(net, x):
    """Kernel launches of one forward."""
    net.set_kernel_timing(x.device, True)
    net.kernel_time()                                    # clear
    net(x)
    torch.cuda.synchronize()
    _, launches, _ = net.kernel_time()
    net.set_kernel_timing(x.device, False)
    return launches
