"""Which kernels did a forward pass of the ARU engine launch?  A plain helper of the GPU tests (no fixtures): the engine's own launch recorder
(asep_aru_profile mode 2, asep_aru_profile_report: include/asep_hip.h) around ONE forward pass through the existing Python helper.

A recorded name is the kernel's rocprofv3 name without "void ", "asep::", blanks and the argument list, every template argument spelled out, and --
in mode 2 -- the layer behind a blank:  "convr_kernel<false,true,true,64> aru_net/featMapG/unet_up_3/convR_2 41x68+21x34+11x17 64->64".
Recording serialises the net on one stream and one lane, so a profile is always taken in a pass of its own: results that a test compares come
from calls made while nothing is recorded."""
import ctypes as C
import json


# attention conv2 (12 -> 16 channels, 4 x 4) of the plain fp32 engine: the dense 12-channel K mapping and the form padded to 16 channels (ASEP_C12=0)
C12_DENSE, C12_PADDED = "conv_mfma_kernel<4,4,1,false,16,false,false,true,2>", "conv_mfma_kernel<4,4,1,false,16,false,false,false,2>"


def launched(graph, image, device="0"):
    """{recorded name: calls} of one forward pass of `image` through `graph` (an AruGraph); recording is off again afterwards"""
    from citlab_article_separation_new_amd import _lib, net_post_processing_helper as helper
    lib = _lib.init_device(int(device))
    h = graph.handle(int(device))
    _lib.check(lib.asep_aru_profile(h, 2), "asep_aru_profile")
    try:
        helper.get_net_output(image, graph, device)
        buf = C.create_string_buffer(1 << 20)
        _lib.check(lib.asep_aru_profile_report(h, buf, len(buf)), "asep_aru_profile_report")
    finally:
        lib.asep_aru_profile(h, 0)
    out = {}
    for rec in json.loads(buf.value.decode()):
        out[rec["kernel"]] = out.get(rec["kernel"], 0) + int(rec["calls"])
    return out


def instance(name):
    """the kernel with its template arguments: the recorded name without the layer text"""
    return name.split(" ", 1)[0]


def base(name):
    """the kernel's base name: what stands in front of '<'"""
    return instance(name).split("<", 1)[0]


def layer(name):
    """the layer text of a mode-2 name ('' where the launcher gives none)"""
    return name.split(" ", 1)[1] if " " in name else ""


def calls(profile, kernel, layer_part=None):
    """launches of `kernel` in a profile: a base name ("convr_kernel") counts every instantiation, a name with '<' that instantiation alone;
    layer_part: only the launches whose layer text contains it"""
    key = instance if "<" in kernel else base
    return sum(n for name, n in profile.items() if key(name) == kernel and (layer_part is None or layer_part in layer(name)))


def kernel_set(profile):
    """the instantiations a pass launched, without the layer texts"""
    return {instance(name) for name, n in profile.items() if n > 0}


def check(profile, present=(), absent=(), what=""):
    """every kernel of `present` launched, none of `absent`; the message names the kernel and lists what ran instead"""
    ran = sorted(kernel_set(profile))
    for k in present:
        assert calls(profile, k) > 0, f"{what}: {k} was not launched; launched: {ran}"
    for k in absent:
        assert calls(profile, k) == 0, f"{what}: {k} was launched ({calls(profile, k)} times) and must not be; launched: {ran}"
