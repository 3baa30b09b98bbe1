# ccall wrappers of include/celeste_detect.h (libceleste_detect.so): source detection on the MI355X.
# Kept apart from CelesteMI355X.jl, whose surface is fixed.  Not executed in this repository's tests (no Julia here):
# tests/test_julia_detect_shim_signatures.py holds every ccall to the header's prototypes.
module CelesteMI355XDetect

const LIB = get(ENV, "CELESTE_MI355X_DETECT_LIB", joinpath(@__DIR__, "..", "celeste.jl_amd", "csrc", "detect", "libceleste_detect.so"))

struct DetectImage            # celeste_detect_image_t
    H::Int32
    W::Int32
    pixels::Ptr{Float32}
    sky::Ptr{Float32}
    nelec_per_nmgy::Ptr{Float32}
end

struct DetectParams           # celeste_detect_params_t
    thresh::Float32
    minarea::Int32
    deblend_nthresh::Int32
    flags::Int32
    deblend_cont::Float64
    lds_max_pixels::Int32
    reserved::Int32
end

version() = ccall((:celeste_detect_version, LIB), Cint, ())
strerror(status) = unsafe_string(ccall((:celeste_detect_strerror, LIB), Cstring, (Cint,), status))

# images: Vector{DetectImage} over column-major Julia arrays transposed to the header's row-major H x W layout
function run(device, images::Vector{DetectImage}, params::DetectParams)
    out = Ref{Ptr{Void}}(C_NULL)
    st = ccall((:celeste_detect_run, LIB), Cint, (Int32, Int32, Ptr{DetectImage}, Ref{DetectParams}, Ptr{Ptr{Void}}),
               device, length(images), images, params, out)
    st == 0 || error("celeste_detect_run: ", strerror(st))
    return out[]
end

result_free(res) = ccall((:celeste_detect_result_free, LIB), Void, (Ptr{Void},), res)

end
