// gpu/gpu.cpp — implementation of the HIP-backed gpu:: layer and the program table that maps
// the reference's program names (src/shaders/config.json) onto C-ABI entry points.
#include "gpu.hpp"
#include <dlfcn.h>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstddef>

#include <map>
#include <mutex>

namespace gpu {

// ---- allocation --------------------------------------------------------------------------------
namespace {
void* default_alloc(size_t bytes, void*) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) throw std::runtime_error{std::string{"hipMalloc failed: "} + hipGetErrorString(e)};
  return p;
}
void default_free(void* p, void*) { (void)hipFree(p); }
AllocFn g_alloc = default_alloc;
FreeFn g_free = default_free;
void* g_alloc_user = nullptr;
}  // namespace

void set_device_allocator(AllocFn alloc, FreeFn free_fn, void* user) {
  g_alloc = alloc ? alloc : default_alloc;
  g_free = free_fn ? free_fn : default_free;
  g_alloc_user = user;
}
void* device_alloc(size_t bytes) {
  void* p = g_alloc(bytes, g_alloc_user);
  if (!p) throw std::runtime_error{"device allocation failed"};
  return p;
}
void device_free(void* ptr) { if (ptr) g_free(ptr, g_alloc_user); }

namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    // rocprofv3 --marker-trace records the ranges of rocprofiler-sdk's ROCTx; libroctx64 is roctracer's (rocprof v1 / v2)
    for (const char* n : {"librocprofiler-sdk-roctx.so.1", "/opt/rocm/lib/librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "/opt/rocm/lib/libroctx64.so.4"}) {
      if (void* h = dlopen(n, RTLD_NOW | RTLD_LOCAL)) {
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (push && pop) return;
        push = nullptr; pop = nullptr;
      }
    }
  }
};
Roctx& roctx() { static Roctx r; return r; }
}  // namespace
void trace_push(const char* name) { if (roctx().push) roctx().push(name); }
void trace_pop() { if (roctx().pop) roctx().pop(); }

void check_status(int rc, const char* what) {
  if (rc != 0) throw std::runtime_error{std::string{what} + ": " + vkr_last_error() + " (code " + std::to_string(rc) + ")"};
}

// ---- images ----------------------------------------------------------------------------------------
uint32_t to_vkr_format(VkFormat fmt) {
  switch (fmt) {
    case VK_FORMAT_D24_UNORM_S8_UINT: return VKR_FMT_D24_UNORM_S8;
    case VK_FORMAT_R16G16_UNORM: return VKR_FMT_RG16_UNORM;
    case VK_FORMAT_R16G16_SFLOAT: return VKR_FMT_RG16_SFLOAT;
    case VK_FORMAT_R8G8B8A8_SRGB: return VKR_FMT_RGBA8_SRGB;
    case VK_FORMAT_R8G8B8A8_UNORM: return VKR_FMT_RGBA8_UNORM;
    case VK_FORMAT_R16G16B16A16_UNORM: return VKR_FMT_RGBA16_UNORM;
    case VK_FORMAT_R16G16B16A16_SFLOAT: return VKR_FMT_RGBA16_SFLOAT;
    case VK_FORMAT_R16_SFLOAT: return VKR_FMT_R16_SFLOAT;
    case VK_FORMAT_R16_UNORM: return VKR_FMT_R16_UNORM;
    case VK_FORMAT_R32_SFLOAT: return VKR_FMT_R32_SFLOAT;
    case VK_FORMAT_R8_UNORM: return VKR_FMT_R8_UNORM;
    case VK_FORMAT_R32G32B32A32_SFLOAT: return VKR_FMT_RGBA32_SFLOAT;
    default: throw std::runtime_error{"Unsupported image format on the post-process path"};
  }
}

static inline uint32_t mip_dim(uint32_t v, uint32_t i) { uint32_t r = v >> i; return r ? r : 1u; }

Image::Image(const ImageInfo& i, const FrameWindow& w) : info{i}, window{w} {
  if (info.mip_levels == 0 || info.mip_levels > VKR_MAX_MIPS) throw std::runtime_error{"Image: bad mip count"};
  if (info.width == 0 || info.height == 0) throw std::runtime_error{"Image: empty extent"};
  const uint32_t bpp = vkr_format_bytes(to_vkr_format(info.format));
  uint64_t off = 0;
  const uint32_t layers = info.array_layers ? info.array_layers : 1;
  for (uint32_t m = 0; m < info.mip_levels; m++) {
    pitch[m] = (mip_dim(info.width, m) * bpp + 255u) & ~255u;  // rows 256-B aligned
    offset[m] = off;
    off += (uint64_t(pitch[m]) * mip_dim(info.height, m) * layers + 255u) & ~uint64_t(255);
  }
  bytes = off;
  base = device_alloc(bytes);
  if (window.full_width == 0) { window.full_width = info.width; window.full_height = info.height; }
}
Image::~Image() { device_free(base); }

vkr_img Image::describe(uint32_t base_mip, uint32_t count) const {
  if (base_mip + count > info.mip_levels || count == 0) throw std::runtime_error{"Image view outside the mip chain"};
  vkr_img d{};
  d.base = (uint8_t*)base + offset[base_mip];
  d.format = to_vkr_format(info.format);
  d.mip_count = count;
  d.width = mip_dim(info.width, base_mip);
  d.height = mip_dim(info.height, base_mip);
  d.full_width = mip_dim(window.full_width, base_mip);
  d.full_height = mip_dim(window.full_height, base_mip);
  d.origin_x = window.origin_x >> base_mip;
  d.origin_y = window.origin_y >> base_mip;
  for (uint32_t m = 0; m < count; m++) {
    d.pitch_bytes[m] = pitch[base_mip + m];
    d.mip_offset[m] = offset[base_mip + m] - offset[base_mip];
  }
  return d;
}

void Image::set_store_rows(uint32_t row0, uint32_t rows) {
  if (rows && (info.mip_levels != 1 || get_array_layers() != 1 || uint64_t(row0) + rows > info.height))
    throw std::runtime_error{"Image::set_store_rows: rows outside the window, or not a single-mip image"};
  store_row0 = rows ? row0 : 0;
  store_rows = rows;
}
vkr_img Image::describe_store(uint32_t base_mip, uint32_t count) const {
  vkr_img d = describe(base_mip, count);
  if (store_rows) {  // (single-mip image: base_mip = 0, count = 1)
    d.base = (uint8_t*)d.base + uint64_t(store_row0) * d.pitch_bytes[0];
    d.origin_y += (int32_t)store_row0;
    d.height = store_rows;
  }
  return d;
}

vkr_img Image::describe_layer(uint32_t layer, uint32_t base_mip, uint32_t count) const {
  if (layer >= get_array_layers()) throw std::runtime_error{"Image layer view outside the array"};
  vkr_img d = describe(base_mip, count);
  auto layer_offset = [&](uint32_t m) { return offset[m] + uint64_t(pitch[m]) * mip_dim(info.height, m) * layer; };
  d.base = (uint8_t*)base + layer_offset(base_mip);
  for (uint32_t m = 0; m < count; m++) d.mip_offset[m] = layer_offset(base_mip + m) - layer_offset(base_mip);
  return d;
}

void Image::upload_mip(uint32_t mip, const void* rows) {
  if (mip >= info.mip_levels) throw std::runtime_error{"Image upload outside the mip chain"};
  const uint32_t bpp = vkr_format_bytes(to_vkr_format(info.format));
  const uint32_t w = mip_dim(info.width, mip), h = mip_dim(info.height, mip);
  hipError_t e = hipMemcpy2D((uint8_t*)base + offset[mip], pitch[mip], rows, size_t(w) * bpp, size_t(w) * bpp, h, hipMemcpyHostToDevice);
  if (e != hipSuccess) throw std::runtime_error{std::string{"image upload failed: "} + hipGetErrorString(e)};
}

Buffer::Buffer(VmaMemoryUsage memory, uint64_t sz, VkBufferUsageFlags usage) : size{sz} {
  dev = device_alloc((sz + 255) & ~uint64_t(255));
  // host shadow: mapped (CPU_TO_GPU) buffers, and uniform buffers — their contents become kernel
  // arguments of the C-ABI call, so the program reads them on the host
  if (memory != VMA_MEMORY_USAGE_GPU_ONLY || (usage & VK_BUFFER_USAGE_UNIFORM_BUFFER_BIT)) shadow.resize(sz);
}
Buffer::~Buffer() { device_free(dev); }
void* Buffer::device_ptr(void* stream) {
  if (dirty && !shadow.empty()) {
    hipError_t e = hipMemcpyAsync(dev, shadow.data(), size, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) throw std::runtime_error{std::string{"buffer upload failed: "} + hipGetErrorString(e)};
    e = hipStreamSynchronize((hipStream_t)stream);  // the shadow is pageable; happens once per write
    if (e != hipSuccess) throw std::runtime_error{std::string{"buffer upload failed: "} + hipGetErrorString(e)};
    dirty = false;
  }
  return dev;
}
BufferPtr create_buffer(VmaMemoryUsage memory, uint64_t size, VkBufferUsageFlags usage) { return std::make_shared<Buffer>(memory, size, usage); }

// ---- samplers ----------------------------------------------------------------------------------------
namespace { std::vector<std::unique_ptr<VkSamplerCreateInfo>> g_samplers; std::mutex g_sampler_lock; }
VkSampler create_sampler(const VkSamplerCreateInfo& info) {
  std::lock_guard<std::mutex> lock{g_sampler_lock};
  for (auto& s : g_samplers)
    if (std::memcmp(s.get(), &info, sizeof(info)) == 0) return (VkSampler)s.get();
  g_samplers.emplace_back(new VkSamplerCreateInfo(info));
  return (VkSampler)g_samplers.back().get();
}
const VkSamplerCreateInfo& sampler_info(VkSampler s) { return *(const VkSamplerCreateInfo*)s; }

// ---- descriptor writes -----------------------------------------------------------------------------------
static SetSlot& slot_of(VkDescriptorSet set, uint32_t binding) {
  if (!set) throw std::runtime_error{"write_set: null descriptor set"};
  auto* obj = (DescriptorSetObject*)set;
  if (binding >= obj->slots.size()) throw std::runtime_error{"write_set: binding out of range"};
  return obj->slots[binding];
}
static const ImageViewObject& view_of(VkImageView v) {
  if (!v) throw std::runtime_error{"write_set: null image view"};
  return *(const ImageViewObject*)v;
}
void write_binding(VkDescriptorSet set, const AccelerationStructBinding& b) {
  auto& s = slot_of(set, b.binding);
  if (!b.tlas) throw std::runtime_error{"write_set: null acceleration structure"};
  s = SetSlot{};
  s.kind = SetSlot::AccelStruct; s.tlas = b.tlas;
}
void write_binding(VkDescriptorSet set, const TextureBinding& b) {
  auto& s = slot_of(set, b.binding);
  s = SetSlot{};
  s.kind = SetSlot::Texture; s.view = view_of(b.view); s.sampler = b.sampler;
}
void write_binding(VkDescriptorSet set, const StorageTextureBinding& b) {
  auto& s = slot_of(set, b.binding);
  s = SetSlot{};
  s.kind = SetSlot::StorageTexture; s.view = view_of(b.view);
}
void write_binding(VkDescriptorSet set, const UBOBinding& b) {
  auto& s = slot_of(set, b.binding);
  s = SetSlot{};
  s.kind = SetSlot::Ubo; s.host_data = b.host; s.host_size = b.size; s.buffer = b.buffer;
}
void write_binding(VkDescriptorSet set, const SSBOBinding& b) {
  auto& s = slot_of(set, b.binding);
  s = SetSlot{};
  s.kind = SetSlot::Ssbo; s.buffer = b.buffer;
}

namespace { std::vector<std::unique_ptr<DescriptorSetObject>> g_long_lived_sets; std::mutex g_set_lock; }
VkDescriptorSet allocate_descriptor_set(VkDescriptorSetLayout, const std::initializer_list<uint32_t>&) {
  std::lock_guard<std::mutex> lock{g_set_lock};
  g_long_lived_sets.emplace_back(new DescriptorSetObject{});
  return (VkDescriptorSet)g_long_lived_sets.back().get();
}
void write_binding(VkDescriptorSet set, const ArrayOfImagesBinding& b) {
  if (!set) throw std::runtime_error{"write_set: null descriptor set"};
  auto* obj = (DescriptorSetObject*)set;
  obj->image_array.clear();
  for (const auto& it : b.images) obj->image_array.push_back(view_of(it.first));
}

// ---- program table ----------------------------------------------------------------------------------------
namespace {
std::map<std::string, ProgramFn>& programs() { static std::map<std::string, ProgramFn> p; return p; }

// `nearest_border`: the one non-default sampler of the path (ssr.cpp:21-28: NEAREST, U clamp-to-border)
vkr_img tex(const LaunchState& st, uint32_t slot, SetSlot::Kind kind, const char* prog, bool nearest_border = false) {
  const SetSlot& s = st.set ? st.set->slots[slot] : SetSlot{};
  if (!st.set || s.kind != kind || !s.view.image)
    throw std::runtime_error{std::string{prog} + ": binding " + std::to_string(slot) + " is not bound as expected"};
  if (kind == SetSlot::Texture) {
    if (!s.sampler) throw std::runtime_error{std::string{prog} + ": binding " + std::to_string(slot) + " has no sampler"};
    const auto& si = sampler_info(s.sampler);
    const bool is_default = si.magFilter == VK_FILTER_LINEAR && si.addressModeU == VK_SAMPLER_ADDRESS_MODE_CLAMP_TO_EDGE;
    const bool is_nearest_border = si.magFilter == VK_FILTER_NEAREST && si.minFilter == VK_FILTER_NEAREST &&
                                   si.addressModeU == VK_SAMPLER_ADDRESS_MODE_CLAMP_TO_BORDER && si.addressModeV == VK_SAMPLER_ADDRESS_MODE_CLAMP_TO_EDGE;
    if (nearest_border ? !is_nearest_border : !is_default)
      throw std::runtime_error{std::string{prog} + ": binding " + std::to_string(slot) + ": sampler not implemented on this path"};
  }
  if (kind == SetSlot::StorageTexture) return s.view.image->describe_store(s.view.range.base_mip, s.view.range.mips_count);
  return s.view.image->describe(s.view.range.base_mip, s.view.range.mips_count);
}
// The Halton(2,3) UBO of AdvancedSSR (advanced_ssr.cpp:54-58: 128 x vec4, xy filled, zw = 0).  The HIP programs want
// cos / sin(2 PI y) in zw (evaluated on the host once instead of per ray, vkr_halton23_fill); a table that arrives as
// the reference builds it is completed here, in the buffer's host shadow, before it is uploaded.
const float* halton_table(Buffer* b, void* stream) {
  const float* h = (const float*)b->host_data();
  const size_t n = b->get_size() / 16;
  bool raw = h != nullptr && n > 0;
  for (size_t i = 0; raw && i < n; i++) raw = h[4 * i + 2] == 0.0f && h[4 * i + 3] == 0.0f;
  if (raw) {
    float* w = (float*)b->get_mapped_ptr();  // marks the shadow dirty: re-uploaded by device_ptr() below
    const float PI = 3.1415926535897932384626433832795f;
    for (size_t i = 0; i < n; i++) {
      const float phi = (2.0f * PI) * w[4 * i + 1];
      w[4 * i + 2] = (float)std::cos((double)phi);
      w[4 * i + 3] = (float)std::sin((double)phi);
    }
  }
  return (const float*)b->device_ptr(stream);
}

template <typename T> const T* ubo(const LaunchState& st, uint32_t slot, const char* prog) {
  const SetSlot& s = st.set ? st.set->slots[slot] : SetSlot{};
  if (!st.set || s.kind != SetSlot::Ubo) throw std::runtime_error{std::string{prog} + ": uniform block " + std::to_string(slot) + " is not bound"};
  const void* data = s.host_data ? s.host_data : (s.buffer ? s.buffer->host_data() : nullptr);
  const uint64_t size = s.host_data ? s.host_size : (s.buffer ? s.buffer->get_size() : 0);
  if (!data || size < sizeof(T)) throw std::runtime_error{std::string{prog} + ": uniform block " + std::to_string(slot) + " is not bound"};
  return (const T*)data;
}
template <typename T> const T* push(const LaunchState& st, const char* prog) {
  if (st.push_size < sizeof(T)) throw std::runtime_error{std::string{prog} + ": push constants missing"};
  return (const T*)st.push;
}
Buffer* ssbo(const LaunchState& st, uint32_t slot, const char* prog) {
  const SetSlot& s = st.set ? st.set->slots[slot] : SetSlot{};
  if (!st.set || s.kind != SetSlot::Ssbo || !s.buffer) throw std::runtime_error{std::string{prog} + ": storage buffer " + std::to_string(slot) + " is not bound"};
  return s.buffer.get();
}
// the Halton(2,3) table of a program, completed and on the device (halton_table)
const float* halton(const LaunchState& st, uint32_t slot, const char* prog) {
  const SetSlot& h = st.set->slots[slot];
  if (h.kind != SetSlot::Ubo || !h.buffer) throw std::runtime_error{std::string{prog} + ": Halton buffer (binding " + std::to_string(slot) + ") is not bound"};
  return halton_table(h.buffer.get(), st.stream);
}
const vkr_accel* accel(const LaunchState& st, uint32_t slot, const char* prog) {
  const SetSlot& as = st.set->slots[slot];
  if (as.kind != SetSlot::AccelStruct || !as.tlas)
    throw std::runtime_error{std::string{prog} + ": acceleration structure (binding " + std::to_string(slot) + ") is not bound"};
  return (const vkr_accel*)as.tlas;
}
// attachment `i` of a graphics program (colour..., depth last) as a one-mip image; `store`: only the rows the frame asked for
// (a tiled frame shades its strip and one row either side, Image::set_store_rows)
vkr_img attachment(const LaunchState& st, size_t i, bool store = false) {
  const ImageViewObject& a = st.attachments[i];
  return store ? a.image->describe_store(a.range.base_mip, 1) : a.image->describe(a.range.base_mip, 1);
}
// the full-screen programs draw into exactly one colour attachment
void expect_one_attachment(const LaunchState& st, const char* prog) {
  if (st.attachments.size() != 1) throw std::runtime_error{std::string{prog} + ": expects one colour attachment"};
}
// the view behind a texture / storage binding, for the programs that look at the image's layers themselves
const ImageViewObject& bound_view(const LaunchState& st, uint32_t slot, SetSlot::Kind kind, const char* prog) {
  if (!st.set || st.set->slots[slot].kind != kind || !st.set->slots[slot].view.image)
    throw std::runtime_error{std::string{prog} + ": binding " + std::to_string(slot) + " is not bound as expected"};
  return st.set->slots[slot].view;
}
// a view of one layer of an array image (or of a plain image) as the C-ABI descriptor of its mips
vkr_img layer_view(const ImageViewObject& v) {
  return v.image->get_array_layers() > 1 ? v.image->describe_layer(v.range.base_layer, v.range.base_mip, v.range.mips_count)
                                         : v.image->describe(v.range.base_mip, v.range.mips_count);
}
std::vector<vkr_img> layers_of(const LaunchState& st, uint32_t slot, SetSlot::Kind kind, const char* prog) {
  const Image& image = *bound_view(st, slot, kind, prog).image;
  std::vector<vkr_img> layers;
  for (uint32_t l = 0; l < image.get_array_layers(); l++) layers.push_back(image.describe_layer(l));
  return layers;
}
// What the three windowed traces bind at the same slots, after the depth at 0 (the head: its window's pyramid levels at 0 and the
// whole-frame pyramid at 10).  Looked up in slot order, so the first unbound slot is the one reported.
struct WindowedTraceImages {
  vkr_img normal, material, rays, occ, pdf, mask, data;
  WindowedTraceImages(const LaunchState& st, const char* prog)
      : normal{tex(st, 1, SetSlot::Texture, prog)}, material{tex(st, 2, SetSlot::Texture, prog)}, rays{tex(st, 5, SetSlot::StorageTexture, prog)},
        occ{tex(st, 6, SetSlot::StorageTexture, prog)}, pdf{tex(st, 7, SetSlot::Texture, prog)}, mask{tex(st, 8, SetSlot::StorageTexture, prog)},
        data{tex(st, 9, SetSlot::StorageTexture, prog)} {}
};
// What the three raster programs hand their kernels: the bound geometry, the host-visible transforms at binding 1, the textures
// of `textures_from` and one vkr_raster_draw per recorded draw_indexed, from the first `push_bytes` bytes of its PushData
// {transform, albedo, mr, flags}; an index the push constants do not carry is 0xFFFFFFFF, no texture.  A program makes the two
// checks where it always made them (its own checks of the attachments lie between them), then builds the scene.
struct RasterScene {
  std::vector<vkr_img> textures;
  std::vector<vkr_raster_draw> draws;
  vkr_raster_scene scene{};
  uint32_t triangles = 0;
  static void expect_geometry(const LaunchState& st, const char* prog) {
    if (!st.vertex_buffer || !st.index_buffer) throw std::runtime_error{std::string{prog} + ": vertex / index buffer not bound"};
  }
  static Buffer* host_transforms(const LaunchState& st, const char* prog) {
    Buffer* transforms = ssbo(st, 1, prog);
    if (!transforms->host_data()) throw std::runtime_error{std::string{prog} + ": the transform buffer must be host-visible on this path"};
    return transforms;
  }
  // `flag_opaque_albedo`: VKR_RASTER_DRAW_OPAQUE_ALBEDO where the discard of the fragment shader cannot fire
  RasterScene(const LaunchState& st, const char* prog, Buffer* transforms, size_t push_bytes, const DescriptorSetObject* textures_from, bool flag_opaque_albedo) {
    if (textures_from)
      for (const auto& v : textures_from->image_array) textures.push_back(v.image->describe(v.range.base_mip, v.range.mips_count));
    for (const auto& d : st.indexed_draws) {
      if (d.push.size() < push_bytes) throw std::runtime_error{std::string{prog} + ": push constants missing"};
      vkr_raster_draw r{};
      std::memcpy(&r, d.push.data(), push_bytes);
      if (push_bytes < 8) r.albedo_index = 0xFFFFFFFFu;
      if (push_bytes < 12) r.mr_index = 0xFFFFFFFFu;
      r.index_offset = d.first_index; r.index_count = d.index_count; r.vertex_offset = (uint32_t)d.vertex_offset;
      if (flag_opaque_albedo && textures_from && r.albedo_index < textures_from->image_array.size() && textures_from->image_array[r.albedo_index].image->alpha_never_zero)
        r.reserved |= VKR_RASTER_DRAW_OPAQUE_ALBEDO;
      triangles += d.index_count / 3u;
      draws.push_back(r);
    }
    scene.vertices = (const vkr_raster_vertex*)st.vertex_buffer->device_ptr(st.stream);
    scene.vertex_count = (uint32_t)(st.vertex_buffer->get_size() / sizeof(vkr_raster_vertex));
    scene.indices = (const uint32_t*)st.index_buffer->device_ptr(st.stream);
    scene.index_count = (uint32_t)(st.index_buffer->get_size() / sizeof(uint32_t));
    scene.transforms = (const vkr_raster_transform*)transforms->host_data();
    scene.transform_count = (uint32_t)(transforms->get_size() / sizeof(vkr_raster_transform));
    scene.draws = draws.data(); scene.draw_count = (uint32_t)draws.size();
    scene.textures = textures.empty() ? nullptr : textures.data(); scene.texture_count = (uint32_t)textures.size();
  }
  RasterScene(const RasterScene&) = delete;  // `scene` points into the vectors
};
// grows a device allocation of the command context: the old one may still be in use on the stream
void* grow_only(void*& memory, uint64_t& have, uint64_t bytes, void* stream) {
  if (bytes > have) {
    if (memory) { (void)hipStreamSynchronize((hipStream_t)stream); device_free(memory); }
    memory = nullptr; have = 0;  // (should the allocation throw)
    memory = device_alloc(bytes);
    have = bytes;
  }
  return memory;
}
}  // namespace

vkr_ssao_params ssao_params_from_block(const void* block, uint64_t bytes) {
  vkr_ssao_params p{};
  if (block) std::memcpy(&p, block, (size_t)std::min<uint64_t>(bytes, sizeof(p)));
  return p;
}

void create_program(const std::string& name, ProgramFn fn) { programs()[name] = std::move(fn); }
bool has_program(const std::string& name) { return programs().count(name) != 0; }
std::vector<std::string> program_names() {
  std::vector<std::string> names;
  for (const auto& p : programs()) names.push_back(p.first);
  return names;
}

void register_hot_path_programs() {
  static std::once_flag once;
  std::call_once(once, [] {
    const auto T = SetSlot::Texture, S = SetSlot::StorageTexture;
    // advanced_ssr/downsample_gbuffer.frag: set {0 depth, 1 normal, 2 velocity}; attachments {normal, velocity, depth mip+1}
    create_program("downsample_gbuffer", [=](LaunchState& st) {
      const char* P = "downsample_gbuffer";
      const SetSlot& ds = st.set->slots[0];
      if (st.attachments.size() != 3) throw std::runtime_error{"downsample_gbuffer: expects 2 colour attachments + depth"};
      const ImageViewObject& dout = st.attachments[2];
      if (ds.kind != T || ds.view.image != dout.image || dout.range.base_mip != ds.view.range.base_mip + 1)
        throw std::runtime_error{"downsample_gbuffer: depth attachment must be the next mip of the sampled depth"};
      vkr_img depth = ds.view.image->describe(ds.view.range.base_mip, 2);
      vkr_img n = tex(st, 1, T, P), v = tex(st, 2, T, P);
      vkr_img on = attachment(st, 0), ov = attachment(st, 1);
      return vkr_downsample_gbuffer(&depth, &n, &v, &on, &ov, st.stream);
    });
    // advanced_ssr/depth_mips.frag: set {0 depth mip i-1}; attachments {depth mip i, i+1, ...}.
    // The reference draws once per mip; bound with several consecutive mips the fused kernel
    // builds the whole run in one go (each mip still the 2x2 min of its parent).
    create_program("depth_mips", [=](LaunchState& st) {
      const SetSlot& ds = st.set->slots[0];
      if (st.attachments.empty()) throw std::runtime_error{"depth_mips: expects at least one depth attachment"};
      if (ds.kind != T) throw std::runtime_error{"depth_mips: binding 0 is not bound as expected"};
      for (size_t i = 0; i < st.attachments.size(); i++) {
        const ImageViewObject& dout = st.attachments[i];
        if (ds.view.image != dout.image || dout.range.base_mip != ds.view.range.base_mip + 1 + i)
          throw std::runtime_error{"depth_mips: attachments must be the consecutive mips after the sampled depth"};
      }
      vkr_img depth = ds.view.image->describe(ds.view.range.base_mip, 1 + (uint32_t)st.attachments.size());
      return vkr_depth_mips(&depth, 0, st.stream);
    });
    // advanced_ssr/regression.comp: set {0 depth (a view of mip 1), 1 planes}; push constants camera_to_world + fovy, aspect,
    // znear, zfar.  The kernel covers the storage image's extent: the groups the reference dispatches beyond it store nothing.
    create_program("tile_regression", [=](LaunchState& st) {
      const char* P = "tile_regression";
      vkr_img depth = tex(st, 0, T, P), planes = tex(st, 1, S, P);
      static_assert(sizeof(vkr_tile_regression_push) == 80, "PushConstants of advanced_ssr/regression.comp");
      return vkr_tile_regression(&depth, &planes, push<vkr_tile_regression_push>(st, P), st.stream);
    });
    // gtao/rt_main.frag: set {0 GTAORTParams, 1 depth, 2 normal, 3 acceleration structure, 4 RandomVectors}; colour attachment raw
    create_program("gtao_rt_main", [=](LaunchState& st) {
      const char* P = "gtao_rt_main";
      expect_one_attachment(st, P);
      vkr_img depth = tex(st, 1, T, P), normal = tex(st, 2, T, P);
      const vkr_accel* scene = accel(st, 3, P);
      const SetSlot& dirs = st.set->slots[4];
      if (dirs.kind != SetSlot::Ubo || !dirs.buffer || dirs.buffer->get_size() < 64 * 16)
        throw std::runtime_error{"gtao_rt_main: random directions (binding 4, 64 x vec4) are not bound"};
      vkr_img out = attachment(st, 0);
      return vkr_gtao_rt_main(ubo<vkr_gtao_rt_params>(st, 0, P), &depth, &normal, scene,
                              (const float*)dirs.buffer->device_ptr(st.stream), &out, push<vkr_gtao_rt_push>(st, P), st.stream);
    });
    create_program("pdf_preintegrate", [=](LaunchState& st) {
      vkr_img out = tex(st, 0, S, "pdf_preintegrate");
      return vkr_pdf_preintegrate(&out, st.stream);
    });
    create_program("sssr_trace", [=](LaunchState& st) {
      const char* P = "sssr_trace";
      vkr_img depth = tex(st, 0, T, P), normal = tex(st, 1, T, P), material = tex(st, 2, T, P);
      vkr_img rays = tex(st, 5, S, P), occ = tex(st, 6, S, P), pdf = tex(st, 7, T, P);
      const float* table = halton(st, 4, P);
      // Two launches where they pay: the rays still marching after step 48 (two of the four compacted rounds: a tenth of them) are
      // parked in the context's workspace and finished by the resume launch, 256 rays of many tiles per block.  Same images bit
      // for bit.  Measured on one MI355X (tools/trace_split_probe.py): 3840x2160 0.259 against 0.272 ms (park after one round
      // 0.280, after three 0.268); 1920x1080 0.105 against 0.094 (a second launch and a memset on a 0.1 ms pass);
      // 7680x4320 1.008 against 1.004; 15360x8640 4.196 against 4.007 — the 80-byte records of the parked rays (17 MB at 4K,
      // 270 MB at 15360x8640) must stay in the caches between the two launches for the resume launch to be cheap.
      const uint64_t n_rays = uint64_t(rays.width) * rays.height;
      if ((vkr_get_switches() & VKR_SWITCH_TRACE_ONE_LAUNCH) || n_rays < (1ull << 20) || n_rays > (6ull << 20))
        return vkr_sssr_trace(&depth, &normal, &material, ubo<vkr_trace_params>(st, 3, P), table, &rays, &occ, &pdf, push<vkr_trace_push>(st, P), st.stream);
      const uint64_t bytes = vkr_sssr_trace_workspace_bytes(rays.width, rays.height);
      return vkr_sssr_trace_split(&depth, &normal, &material, ubo<vkr_trace_params>(st, 3, P), table, &rays, &occ, &pdf, push<vkr_trace_push>(st, P),
                                  st.require_workspace(bytes), bytes, 2u, st.stream);
    });
    create_program("sssr_trace_windowed", [=](LaunchState& st) {  // multi-GPU variant (include/vkr_postfx.h), bindings 0..9
      const char* P = "sssr_trace_windowed";
      vkr_img depth = tex(st, 0, T, P);
      WindowedTraceImages w{st, P};
      const float* table = halton(st, 4, P);
      return vkr_sssr_trace_windowed(&depth, &w.normal, &w.material, ubo<vkr_trace_params>(st, 3, P), table, &w.rays, &w.occ, &w.pdf, &w.mask, &w.data,
                                     push<vkr_trace_window_push>(st, P), st.stream);
    });
    // the windowed trace in two tasks (include/vkr_postfx.h): bindings of sssr_trace_windowed, the head with the window's own
    // pyramid levels at 0 and the whole-frame pyramid (extents only) at 10; both use the context's workspace
    create_program("sssr_trace_windowed_head", [=](LaunchState& st) {
      const char* P = "sssr_trace_windowed_head";
      vkr_img local = tex(st, 0, T, P), frame = tex(st, 10, T, P);
      WindowedTraceImages w{st, P};
      const float* table = halton(st, 4, P);
      const uint64_t bytes = vkr_sssr_trace_workspace_bytes(w.rays.width, w.rays.height);
      return vkr_sssr_trace_windowed_head(&local, &frame, &w.normal, &w.material, ubo<vkr_trace_params>(st, 3, P), table, &w.rays, &w.occ, &w.pdf, &w.mask,
                                          &w.data, push<vkr_trace_window_push>(st, P), st.require_workspace(bytes), bytes, 2u, st.stream);
    });
    create_program("sssr_trace_windowed_resume", [=](LaunchState& st) {
      const char* P = "sssr_trace_windowed_resume";
      vkr_img depth = tex(st, 0, T, P);
      WindowedTraceImages w{st, P};
      const float* table = halton(st, 4, P);
      const uint64_t bytes = vkr_sssr_trace_workspace_bytes(w.rays.width, w.rays.height);
      if (st.workspace_bytes < bytes) throw std::runtime_error{"sssr_trace_windowed_resume: no head launch has filled the workspace"};
      return vkr_sssr_trace_windowed_resume(&depth, &w.normal, &w.material, ubo<vkr_trace_params>(st, 3, P), table, &w.rays, &w.occ, &w.pdf, &w.mask,
                                            &w.data, push<vkr_trace_window_push>(st, P), st.workspace, bytes, st.stream);
    });
    create_program("sssr_filter", [=](LaunchState& st) {
      const char* P = "sssr_filter";
      vkr_img rays = tex(st, 0, T, P), depth = tex(st, 1, T, P), albedo = tex(st, 2, T, P), normal = tex(st, 3, T, P);
      vkr_img material = tex(st, 4, T, P), out = tex(st, 5, S, P);
      return vkr_sssr_filter(&rays, &depth, &albedo, &normal, &material, &out, ubo<vkr_trace_params>(st, 6, P),
                             push<vkr_filter_push>(st, P), st.stream);
    });
    create_program("sssr_blur", [=](LaunchState& st) {
      const char* P = "sssr_blur";
      vkr_img depth = tex(st, 0, T, P), normal = tex(st, 1, T, P), refl = tex(st, 2, T, P), material = tex(st, 3, T, P);
      vkr_img history = tex(st, 4, T, P), velocity = tex(st, 5, T, P), hdepth = tex(st, 6, T, P), out = tex(st, 7, S, P);
      return vkr_sssr_blur(&depth, &normal, &refl, &material, &history, &velocity, &hdepth, &out,
                           ubo<vkr_reproject_params>(st, 8, P), push<vkr_blur_push>(st, P), st.stream);
    });
    create_program("gtao_compute_main", [=](LaunchState& st) {
      const char* P = "gtao_compute_main";
      vkr_img depth = tex(st, 0, T, P), normal = tex(st, 2, T, P), material = tex(st, 3, T, P), pdf = tex(st, 4, T, P);
      vkr_img out = tex(st, 5, S, P);
      return vkr_gtao_main(&depth, ubo<vkr_gtao_params>(st, 1, P), &normal, &material, &pdf, &out, push<vkr_gtao_push>(st, P), st.stream);
    });
    create_program("gtao_filter", [=](LaunchState& st) {
      const char* P = "gtao_filter";
      vkr_img depth = tex(st, 0, T, P), raw = tex(st, 1, T, P), out = tex(st, 2, S, P);
      return vkr_gtao_filter(&depth, &raw, &out, push<vkr_gtao_filter_push>(st, P), st.stream);
    });
    create_program("gtao_accumulate", [=](LaunchState& st) {
      const char* P = "gtao_accumulate";
      vkr_img depth = tex(st, 0, T, P), pdepth = tex(st, 1, T, P), ao = tex(st, 2, T, P), out = tex(st, 3, S, P);
      vkr_img velocity = tex(st, 4, T, P), history = tex(st, 5, T, P);
      return vkr_gtao_accumulate(&depth, &pdepth, &ao, &out, &velocity, &history, ubo<vkr_gtao_accum_params>(st, 6, P),
                                 push<vkr_gtao_accum_push>(st, P), st.stream);
    });
    create_program("taa_resolve", [=](LaunchState& st) {
      const char* P = "taa_resolve";
      vkr_img hist = tex(st, 0, T, P), hdepth = tex(st, 1, T, P), depth = tex(st, 2, T, P), velocity = tex(st, 3, T, P);
      vkr_img color = tex(st, 4, T, P), out = tex(st, 5, S, P);
      return vkr_taa_resolve(&hist, &hdepth, &depth, &velocity, &color, &out, ubo<vkr_reproject_params>(st, 6, P), st.stream);
    });
    // ssr/shader.frag: set {0 normal, 1 depth (nearest/border sampler), 2 frame, 3 SSRParams, 4 material}; attachment {out}
    create_program("ssr", [=](LaunchState& st) {
      const char* P = "ssr";
      expect_one_attachment(st, P);
      vkr_img normal = tex(st, 0, T, P), depth = tex(st, 1, T, P, true), frame = tex(st, 2, T, P), material = tex(st, 4, T, P);
      vkr_img out = attachment(st, 0);
      return vkr_ssr(&normal, &depth, &frame, ubo<vkr_ssr_params>(st, 3, P), &material, &out, st.stream);
    });
    create_program("brdf_preintegrate", [=](LaunchState& st) {
      const float* table = halton(st, 0, "brdf_preintegrate");
      vkr_img out = tex(st, 1, S, "brdf_preintegrate");
      return vkr_brdf_preintegrate(table, &out, st.stream);
    });
    // defered_shading/shader.frag: set {0 albedo, 1 normal, 2 material, 3 depth, 4 Constants, 5 shadow (unused), 6 occlusion, 7 brdf, 8 reflections}
    create_program("defered_shading", [=](LaunchState& st) {
      const char* P = "defered_shading";
      expect_one_attachment(st, P);
      vkr_img albedo = tex(st, 0, T, P), normal = tex(st, 1, T, P), material = tex(st, 2, T, P), depth = tex(st, 3, T, P);
      vkr_img occlusion = tex(st, 6, T, P), brdf = tex(st, 7, T, P), refl = tex(st, 8, T, P);
      vkr_img out = attachment(st, 0, true);  // the rows the frame asked for
      return vkr_defered_shading(&albedo, &normal, &material, &depth, ubo<vkr_shading_params>(st, 4, P), &occlusion, &brdf, &refl, &out,
                                 push<vkr_shading_push>(st, P), st.stream);
    });
    // the same set plus {9 shadow mask}: DeferedShadingPass::draw_shadowed
    create_program("defered_shading_shadowed", [=](LaunchState& st) {
      const char* P = "defered_shading_shadowed";
      expect_one_attachment(st, P);
      vkr_img albedo = tex(st, 0, T, P), normal = tex(st, 1, T, P), material = tex(st, 2, T, P), depth = tex(st, 3, T, P);
      vkr_img occlusion = tex(st, 6, T, P), brdf = tex(st, 7, T, P), refl = tex(st, 8, T, P), mask = tex(st, 9, T, P);
      vkr_img out = attachment(st, 0, true);
      return vkr_defered_shading_shadowed(&albedo, &normal, &material, &depth, ubo<vkr_shading_params>(st, 4, P), &occlusion, &brdf, &refl, &mask,
                                          &out, push<vkr_shading_push>(st, P), st.stream);
    });
    // ---- tile-classified trace ----
    create_program("sssr_classification", [=](LaunchState& st) {
      const char* P = "sssr_classification";
      vkr_img material = tex(st, 0, T, P);
      return vkr_sssr_classification(&material, (int32_t*)ssbo(st, 1, P)->device_ptr(st.stream), (int32_t*)ssbo(st, 2, P)->device_ptr(st.stream),
                                     (uint32_t*)ssbo(st, 3, P)->device_ptr(st.stream), (uint32_t*)ssbo(st, 4, P)->device_ptr(st.stream),
                                     push<vkr_classification_push>(st, P), st.stream);
    });
    create_program("sssr_trace_indirect", [=](LaunchState& st) {
      const char* P = "sssr_trace_indirect";
      if (!st.indirect) throw std::runtime_error{"sssr_trace_indirect: must be launched with dispatch_indirect"};
      vkr_img depth = tex(st, 0, T, P), normal = tex(st, 1, T, P), material = tex(st, 2, T, P), rays = tex(st, 5, S, P);
      const float* table = halton(st, 4, P);
      Buffer* tiles = ssbo(st, 6, P);
      return vkr_sssr_trace_indirect(&depth, &normal, &material, ubo<vkr_trace_params>(st, 3, P), table, &rays,
                                     (const int32_t*)tiles->device_ptr(st.stream), (const uint32_t*)st.indirect->device_ptr(st.stream),
                                     (uint32_t)(tiles->get_size() / sizeof(int32_t)), push<vkr_trace_indirect_push>(st, P), st.stream);
    });
    // ---- G-buffer raster stage: gbuf/opaque_taa.{vert,frag} ----
    // set 0 {0 GbufConst, 1 transforms (pairs of mat4: model, normal)}, set 1 {0 material textures[]}; vertex + index
    // buffers; one recorded draw_indexed per primitive with PushData {transform, albedo, mr, flags}; attachments
    // {albedo, normal, material, velocity, depth}, cleared.
    create_program("gbuf_opaque_taa", [=](LaunchState& st) {
      const char* P = "gbuf_opaque_taa";
      if (st.attachments.size() != 5) throw std::runtime_error{"gbuf_opaque_taa: expects 4 colour attachments + depth"};
      if (!st.cleared_color || !st.cleared_depth) throw std::runtime_error{"gbuf_opaque_taa: attachments must be cleared (colour 0, depth 1)"};
      RasterScene::expect_geometry(st, P);
      Buffer* transforms = RasterScene::host_transforms(st, P);
      vkr_img albedo = attachment(st, 0), normal = attachment(st, 1), material = attachment(st, 2), velocity = attachment(st, 3), depth = attachment(st, 4);
      // PushData {transform, albedo, mr, flags}; flagged: the draws for which the discard of opaque_taa.frag:32-34 cannot fire
      const RasterScene raster{st, P, transforms, 16, st.set1, true};
      return vkr_raster_gbuffer(&raster.scene, ubo<vkr_gbuf_const>(st, 0, P), &albedo, &normal, &material, &velocity, &depth,
                                st.scratch, st.scratch_bytes, st.stream);
    });
    // ---- shadow map (scene_renderer.cpp:222-274): shadows/default.{vert,frag} ----
    // set 0 {0 ShadowConst {mat4 mvp}, 1 transforms (pairs of mat4: model, normal)}; vertex + index buffers; one recorded
    // draw_indexed per primitive with a 4-byte push constant transform_index; one depth attachment (a layer of a square D24S8
    // image), cleared to 1.
    create_program("default_shadow", [=](LaunchState& st) {
      const char* P = "default_shadow";
      if (st.attachments.size() != 1) throw std::runtime_error{"default_shadow: expects one depth attachment"};
      if (!st.cleared_depth) throw std::runtime_error{"default_shadow: the depth attachment must be cleared (depth 1)"};
      RasterScene::expect_geometry(st, P);
      Buffer* transforms = RasterScene::host_transforms(st, P);
      const ImageViewObject& depth = st.attachments[0];
      if (depth.range.base_mip != 0) throw std::runtime_error{"default_shadow: the depth attachment must be mip 0 of a layer"};
      if (st.fb_width != depth.image->get_info().width || st.fb_height != depth.image->get_info().height)
        throw std::runtime_error{"default_shadow: the framebuffer must cover the (square) depth attachment"};
      const vkr_img layer = depth.image->get_array_layers() > 1 ? depth.image->describe_layer(depth.range.base_layer, 0, 1) : depth.image->describe(0, 1);
      const RasterScene raster{st, P, transforms, 4, nullptr, false};  // the push constant is transform_index: no textures
      static_assert(sizeof(vkr_mat4) == 64, "ShadowConst of shadows/default.vert");
      if (st.scratch_bytes < vkr_default_shadow_scratch_bytes(layer.width, 1, raster.triangles)) throw std::runtime_error{"default_shadow: no scratch (CmdContext::require_scratch)"};
      return vkr_default_shadow(&raster.scene, ubo<vkr_mat4>(st, 0, P), &layer, 1, st.scratch, st.scratch_bytes, st.stream);
    });
    // ---- octahedral probes (probe_renderer.cpp): cubemap_probe, cube2oct, probe_downsample, trace_probe ----
    // cubemap_probe/shader.{vert,frag}: set 0 {0 ShaderUbo {projection, camera}, 1 transforms, 2 material textures[], 3 sampler};
    // vertex + index buffers; one draw_indexed per primitive with PushData {transform, albedo}; attachments {cube colour layer,
    // cube distance layer, depth}, cleared to (100, 0, 0, 0) and 1.  One render pass per face, faces 0..5 in order.
    create_program("cubemap_probe", [=](LaunchState& st) {
      const char* P = "cubemap_probe";
      struct ShaderUbo { float projection[16], camera[16]; };
      if (st.attachments.size() != 3) throw std::runtime_error{"cubemap_probe: expects colour, distance and depth attachments"};
      if (!st.cleared_color || !st.cleared_depth || st.clear_color[0] != 100.f)
        throw std::runtime_error{"cubemap_probe: attachments must be cleared (colour (100, 0, 0, 0), depth 1)"};
      RasterScene::expect_geometry(st, P);
      const ImageViewObject &color = st.attachments[0], &distance = st.attachments[1];
      const uint32_t side = color.range.base_layer;
      if (color.image->get_array_layers() != 6 || distance.image->get_array_layers() != 6 || distance.range.base_layer != side || side >= 6)
        throw std::runtime_error{"cubemap_probe: the colour and distance attachments must be the same layer of two cube images"};
      const ShaderUbo* u = ubo<ShaderUbo>(st, 0, P);
      // the view of face `side` is lookAt(pos, pos + fwd, up) of calc_matrix: a signed permutation R and t = -R pos, so pos = -R^T t
      float pos[3];
      for (int k = 0; k < 3; k++) pos[k] = 0.f - ((u->camera[4 * k + 0] * u->camera[12] + u->camera[4 * k + 1] * u->camera[13]) + u->camera[4 * k + 2] * u->camera[14]);
      if (side == 0) { st.cube = LaunchState::CubeBatch{}; std::memcpy(st.cube.pos, pos, sizeof(pos)); st.cube.color = color.image; st.cube.distance = distance.image; st.cube.draws = st.indexed_draws.size(); }
      if (st.cube.faces != side || st.cube.color != color.image || st.cube.distance != distance.image || st.cube.draws != st.indexed_draws.size() ||
          pos[0] != st.cube.pos[0] || pos[1] != st.cube.pos[1] || pos[2] != st.cube.pos[2])
        throw std::runtime_error{"cubemap_probe: the six faces of a cube are drawn in order 0..5, from one position, with the same draws"};
      st.cube.faces = side + 1;
      if (side != 5) return 0;
      st.cube.faces = 0;
      // PushData {transform_index, albedo_index}; flagged: the draws for which the discard of shader.frag cannot fire
      const RasterScene raster{st, P, RasterScene::host_transforms(st, P), 8, st.set, true};
      vkr_img cc[6], cd[6];
      for (uint32_t f = 0; f < 6; f++) { cc[f] = color.image->describe_layer(f); cd[f] = distance.image->describe_layer(f); }
      return vkr_cubemap_probe(&raster.scene, pos, cc, cd, st.scratch, st.scratch_bytes, st.stream);
    });
    // cube2oct/shader.comp: set {0 cube colour (cube view), 1 cube distance (cube view), 2 oct colour (storage, one layer), 3 oct
    // depth (storage, mip 0 of one layer)}
    create_program("cube2oct", [=](LaunchState& st) {
      const char* P = "cube2oct";
      const ImageViewObject &c = bound_view(st, 0, T, P), &d = bound_view(st, 1, T, P);
      if (c.image->get_array_layers() != 6 || d.image->get_array_layers() != 6) throw std::runtime_error{"cube2oct: bindings 0 and 1 must be cube images"};
      vkr_img cc[6], cd[6];
      for (uint32_t f = 0; f < 6; f++) { cc[f] = c.image->describe_layer(f); cd[f] = d.image->describe_layer(f); }
      vkr_img oc = layer_view(bound_view(st, 2, S, P)), od = layer_view(bound_view(st, 3, S, P));
      return vkr_cube2oct(cc, cd, &oc, &od, st.stream);
    });
    // probe_downsample/shader.frag: set {0 depth mip i - 1 of one layer}; colour attachment: mip i of the same layer
    create_program("probe_downsample", [=](LaunchState& st) {
      const char* P = "probe_downsample";
      expect_one_attachment(st, P);
      const ImageViewObject &src = bound_view(st, 0, T, P), &dst = st.attachments[0];
      if (src.image != dst.image || dst.range.base_mip != src.range.base_mip + 1 || dst.range.base_layer != src.range.base_layer)
        throw std::runtime_error{"probe_downsample: the attachment must be the next mip of the sampled layer"};
      vkr_img two = src.image->get_array_layers() > 1 ? src.image->describe_layer(src.range.base_layer, src.range.base_mip, 2)
                                                      : src.image->describe(src.range.base_mip, 2);
      return vkr_probe_downsample(&two, st.stream);
    });
    // trace_probe/shader.comp: set {0 depth, 1 normal, 2 probe colour array, 3 probe depth array (all mips), 4 Constants, 5 out}
    create_program("trace_probe", [=](LaunchState& st) {
      const char* P = "trace_probe";
      vkr_img depth = tex(st, 0, T, P), normal = tex(st, 1, T, P), out = tex(st, 5, S, P);
      const ImageViewObject &pc = bound_view(st, 2, T, P), &pd = bound_view(st, 3, T, P);
      const uint32_t layers = pc.image->get_array_layers();
      if (pd.image->get_array_layers() != layers) throw std::runtime_error{"trace_probe: the probe colour and depth arrays differ in layers"};
      std::vector<vkr_img> cl(layers), dl(layers);
      for (uint32_t l = 0; l < layers; l++) { cl[l] = pc.image->describe_layer(l, 0, 1); dl[l] = pd.image->describe_layer(l, 0, pd.image->get_mip_levels()); }
      static_assert(sizeof(vkr_probe_trace_consts) == 116, "Constants of trace_probe/shader.comp");
      return vkr_trace_probe(&depth, &normal, cl.data(), dl.data(), layers, ubo<vkr_probe_trace_consts>(st, 4, P), &out, st.stream);
    });
    // ---- SSAO (ssao.cpp) ----
    // ssao/shader.frag: set {0 depth, 1 SSAOParams}; colour attachment occlusion.  The block is taken as the shader would read
    // it, whatever size the host struct has (ssao_params_from_block).
    create_program("ssao", [=](LaunchState& st) {
      const char* P = "ssao";
      expect_one_attachment(st, P);
      vkr_img depth = tex(st, 0, T, P);
      const SetSlot& b = st.set->slots[1];
      const void* data = b.host_data ? b.host_data : (b.buffer ? b.buffer->host_data() : nullptr);
      const uint64_t size = b.host_data ? b.host_size : (b.buffer ? b.buffer->get_size() : 0);
      if (b.kind != SetSlot::Ubo || !data || size < 80) throw std::runtime_error{"ssao: uniform block 1 is not bound"};
      static_assert(sizeof(vkr_ssao_params) == 336 && offsetof(vkr_ssao_params, samples) == 80, "SSAOParams of ssao/shader.frag (std140)");
      const vkr_ssao_params params = ssao_params_from_block(data, size);
      vkr_img out = attachment(st, 0);
      return vkr_ssao(&depth, &params, &out, st.stream);
    });
    // ---- shadow mask (ShadowMaskPass; no reference program) ----
    // set {0 depth (mip 0), 1 the shadow array (every layer), 2 vkr_shadow_mask_params, 3 the mask (storage)}
    create_program("shadow_mask", [=](LaunchState& st) {
      const char* P = "shadow_mask";
      vkr_img depth = tex(st, 0, T, P), out = tex(st, 3, S, P);
      const ImageViewObject& maps = bound_view(st, 1, T, P);
      static_assert(sizeof(vkr_shadow_mask_params) == 352, "vkr_shadow_mask_params: five matrices and eight words");
      const vkr_shadow_mask_params* params = ubo<vkr_shadow_mask_params>(st, 2, P);
      if (params->layer_count < 1 || params->layer_count > 4 || params->layer_count > maps.image->get_array_layers())
        throw std::runtime_error{"shadow_mask: layer_count " + std::to_string(params->layer_count) + " of a shadow map with " +
                                 std::to_string(maps.image->get_array_layers()) + " layers"};
      vkr_img layers[4];
      for (uint32_t l = 0; l < params->layer_count; l++) layers[l] = maps.image->describe_layer(l, 0, 1);
      return vkr_shadow_mask(&depth, layers, params, &out, st.stream);
    });
    // ---- what a program that looks at hits binds besides its images: the structure, its attribute table, the textures ----
    struct HitTable {
      const vkr_accel* accel;
      const vkr_hit_attrib* attribs;
      uint32_t attrib_count;
      std::vector<vkr_img> textures;
      uint32_t opaque_mask;  // bit i: no texel of textures[i] has alpha 0 (Image::alpha_never_zero, what VKR_RASTER_DRAW_OPAQUE_ALBEDO comes from)
    };
    auto hit_table = [](LaunchState& st, uint32_t accel_slot, uint32_t attrib_slot, const char* P) {
      HitTable h {};
      h.accel = accel(st, accel_slot, P);
      const SetSlot& at = st.set->slots[attrib_slot];
      if (at.kind != SetSlot::Ubo || !at.buffer) throw std::runtime_error{std::string{P} + ": attribute table (binding " + std::to_string(attrib_slot) + ") is not bound"};
      for (const auto& v : st.set->image_array) {
        if (v.image->alpha_never_zero && h.textures.size() < 32) h.opaque_mask |= 1u << h.textures.size();
        h.textures.push_back(v.image->describe(v.range.base_mip, v.range.mips_count));
      }
      // the table of an empty scene still holds one (unused) record: a buffer has no size 0
      uint32_t triangles = 0;
      if (vkr_accel_info(h.accel, nullptr, &triangles) != 0) throw std::runtime_error{std::string{P} + ": " + vkr_last_error()};
      const uint64_t records = at.buffer->get_size() / sizeof(vkr_hit_attrib);
      h.attribs = (const vkr_hit_attrib*)at.buffer->device_ptr(st.stream);
      h.attrib_count = records >= triangles ? triangles : (uint32_t)records;
      return h;
    };
    // the cutout block of a _cutout program, with the bits of the textures that cannot make a hole added to its mask
    auto cutout_block = [=](LaunchState& st, uint32_t slot, const HitTable& h, const char* P) {
      static_assert(sizeof(vkr_ray_cutout) == 8, "vkr_ray_cutout: two words");
      vkr_ray_cutout c = *ubo<vkr_ray_cutout>(st, slot, P);
      c.opaque_texture_mask |= h.opaque_mask;
      return c;
    };
    // the area lights of a _soft program: the block (its samples pointer is not read) and the sample table behind it
    auto soft_block = [=](LaunchState& st, uint32_t slot, uint32_t table_slot, const char* P) {
      static_assert(sizeof(vkr_shadow_rt_soft) == 40, "vkr_shadow_rt_soft: four radii, two words, a pointer and two words");
      vkr_shadow_rt_soft soft = *ubo<vkr_shadow_rt_soft>(st, slot, P);
      const SetSlot& table = st.set->slots[table_slot];
      if (table.kind != SetSlot::Ubo || !table.buffer) throw std::runtime_error{std::string{P} + ": sample table (binding " + std::to_string(table_slot) + ") is not bound"};
      if (table.buffer->get_size() < sizeof(float) * 2 * (uint64_t)soft.sample_count * soft.pattern_side * soft.pattern_side)
        throw std::runtime_error{std::string{P} + ": the sample table is smaller than sample_count x pattern_side^2 pairs"};
      soft.samples = (const float*)table.buffer->device_ptr(st.stream);
      return soft;
    };
    // ---- ray-traced shadow mask (ShadowMaskPass::run_rt; no reference program), in four programs: {cutouts, soft} ----
    // "shadow_mask_rt": set {0 depth (mip 0), 1 normal, 2 acceleration structure, 3 vkr_shadow_rt_params, 4 the mask (storage)}: the
    // C-ABI's order;
    // "shadow_mask_rt_cutout" (the rays see alpha cutouts): the same and {5 the attribute table, 6 vkr_ray_cutout, 7 the scene's
    // textures[]};
    // "shadow_mask_rt_soft" (area lights, after update_rt_soft): the set of "shadow_mask_rt", 5 vkr_shadow_rt_soft, 6 the sample table;
    // "shadow_mask_rt_soft_cutout": the set of "shadow_mask_rt_cutout", 8 vkr_shadow_rt_soft, 9 the sample table
    for (const bool cutouts : {false, true})
      for (const bool soft : {false, true}) {
        const char* P = cutouts ? (soft ? "shadow_mask_rt_soft_cutout" : "shadow_mask_rt_cutout") : (soft ? "shadow_mask_rt_soft" : "shadow_mask_rt");
        create_program(P, [=](LaunchState& st) {
          vkr_img depth = tex(st, 0, T, P), normal = tex(st, 1, T, P), out = tex(st, 4, S, P);
          static_assert(sizeof(vkr_shadow_rt_params) == 160, "vkr_shadow_rt_params: a matrix, four floats, four lights and four words");
          if (!cutouts) {
            const vkr_accel* scene = accel(st, 2, P);
            if (!soft) return vkr_shadow_mask_rt(&depth, &normal, scene, ubo<vkr_shadow_rt_params>(st, 3, P), &out, st.stream);
            const vkr_shadow_rt_soft lights = soft_block(st, 5, 6, P);
            return vkr_shadow_mask_rt_soft(&depth, &normal, scene, ubo<vkr_shadow_rt_params>(st, 3, P), &lights, &out, st.stream);
          }
          const HitTable h = hit_table(st, 2, 5, P);
          const vkr_ray_cutout c = cutout_block(st, 6, h, P);
          const vkr_shadow_rt_soft lights = soft ? soft_block(st, 8, 9, P) : vkr_shadow_rt_soft{};
          const uint32_t count = (uint32_t)h.textures.size();
          const uint64_t bytes = vkr_accel_cutout_scratch_bytes(count);
          const vkr_img* textures = h.textures.empty() ? nullptr : h.textures.data();
          if (!soft)
            return vkr_shadow_mask_rt_cutout(&depth, &normal, h.accel, h.attribs, h.attrib_count, textures, count, ubo<vkr_shadow_rt_params>(st, 3, P), &c, &out,
                                             st.require_workspace(bytes), bytes, st.stream);
          return vkr_shadow_mask_rt_soft_cutout(&depth, &normal, h.accel, h.attribs, h.attrib_count, textures, count, ubo<vkr_shadow_rt_params>(st, 3, P), &c,
                                                &lights, &out, st.require_workspace(bytes), bytes, st.stream);
        });
      }
    // ---- ray-traced reflections (AdvancedSSR::run_reflections_rt_pass; no reference program) ----
    // set {0 depth (mip 0 of the view), 1 normal, 2 rays (bound only in fill mode), 3 acceleration structure, 4 the attribute table,
    // 5 vkr_reflect_rt_params, 6 reflections (storage), 7 the scene's textures[]}; the texture table goes into the context's workspace.
    // "reflections_rt_cutout": the same set and 8 vkr_ray_cutout.
    // Lit hits: a set that also binds 9 the normal table (one vkr_hit_normal per record of the attribute table) and
    // 10 vkr_reflect_lights makes either program record vkr_reflections_rt_lit / vkr_reflections_rt_lit_cutout: "reflections_rt_lit"
    // and "reflections_rt_lit_cutout" are the same two programs on the larger set, not further rows of the table
    for (const bool cutouts : {false, true})
      create_program(cutouts ? "reflections_rt_cutout" : "reflections_rt", [=](LaunchState& st) {
        const char* P = cutouts ? "reflections_rt_cutout" : "reflections_rt";
        vkr_img depth = tex(st, 0, T, P), normal = tex(st, 1, T, P), out = tex(st, 6, S, P);
        static_assert(sizeof(vkr_reflect_rt_params) == 112, "vkr_reflect_rt_params: a matrix, eight floats / words, the flags and three words");
        const vkr_reflect_rt_params* params = ubo<vkr_reflect_rt_params>(st, 5, P);
        vkr_img rays{};
        const bool fill = (params->flags & VKR_REFLECT_RT_FILL_MISSES) != 0;
        if (fill) rays = tex(st, 2, T, P);
        const HitTable h = hit_table(st, 3, 4, P);
        const uint32_t count = (uint32_t)h.textures.size();
        const uint64_t bytes = vkr_reflections_rt_scratch_bytes(count);
        const vkr_img* textures = h.textures.empty() ? nullptr : h.textures.data();
        if (st.set->slots[10].kind == SetSlot::Ubo) {  // lit
          const char* L = cutouts ? "reflections_rt_lit_cutout" : "reflections_rt_lit";
          const SetSlot& nt = st.set->slots[9];
          if (nt.kind != SetSlot::Ubo || !nt.buffer) throw std::runtime_error{std::string{L} + ": normal table (binding 9) is not bound"};
          if (nt.buffer->get_size() < sizeof(vkr_hit_normal) * (uint64_t)h.attrib_count) throw std::runtime_error{std::string{L} + ": the normal table is smaller than the attribute table"};
          const vkr_hit_normal* normals = (const vkr_hit_normal*)nt.buffer->device_ptr(st.stream);
          static_assert(sizeof(vkr_reflect_lights) == 176, "vkr_reflect_lights: nine float4 and eight words");
          const vkr_reflect_lights* lights = ubo<vkr_reflect_lights>(st, 10, L);
          if (!cutouts)
            return vkr_reflections_rt_lit(&depth, &normal, fill ? &rays : nullptr, h.accel, h.attribs, h.attrib_count, normals, h.attrib_count, textures, count,
                                          params, lights, &out, st.require_workspace(bytes), bytes, st.stream);
          const vkr_ray_cutout c = cutout_block(st, 8, h, L);
          return vkr_reflections_rt_lit_cutout(&depth, &normal, fill ? &rays : nullptr, h.accel, h.attribs, h.attrib_count, normals, h.attrib_count, textures,
                                               count, params, lights, &c, &out, st.require_workspace(bytes), bytes, st.stream);
        }
        if (!cutouts)
          return vkr_reflections_rt(&depth, &normal, fill ? &rays : nullptr, h.accel, h.attribs, h.attrib_count, textures, count, params, &out,
                                    st.require_workspace(bytes), bytes, st.stream);
        const vkr_ray_cutout c = cutout_block(st, 8, h, P);
        return vkr_reflections_rt_cutout(&depth, &normal, fill ? &rays : nullptr, h.accel, h.attribs, h.attrib_count, textures, count, params, &c, &out,
                                         st.require_workspace(bytes), bytes, st.stream);
      });
    // ---- backbuffer (backbuffer_subpass2.cpp) ----
    // texdraw/shader.frag: set {0 target_tex}; push constants flags; colour attachment the backbuffer.  The clear to 0 the
    // reference records first is covered by the triangle and not executed.
    create_program("texdraw", [=](LaunchState& st) {
      const char* P = "texdraw";
      expect_one_attachment(st, P);
      vkr_img target_tex = tex(st, 0, T, P);
      static_assert(sizeof(vkr_texdraw_push) == 4, "Constants of texdraw/shader.frag");
      vkr_img backbuffer = attachment(st, 0);
      return vkr_texdraw(&target_tex, &backbuffer, push<vkr_texdraw_push>(st, P), st.stream);
    });
    // ---- dormant GTAO variants ----
    // gtao/main.frag: set {0 depth, 1 GTAOParams, 2 normal}; colour attachment raw
    create_program("gtao_main", [=](LaunchState& st) {
      const char* P = "gtao_main";
      expect_one_attachment(st, P);
      vkr_img depth = tex(st, 0, T, P), normal = tex(st, 2, T, P);
      vkr_img out = attachment(st, 0);
      return vkr_gtao_main_graphics(&depth, ubo<vkr_gtao_params>(st, 1, P), &normal, &out, push<vkr_gtao_gfx_push>(st, P), st.stream);
    });
    create_program("gtao_reproject", [=](LaunchState& st) {
      const char* P = "gtao_reproject";
      vkr_img depth = tex(st, 1, T, P), pdepth = tex(st, 2, T, P), ao = tex(st, 3, T, P), pao = tex(st, 4, T, P), out = tex(st, 5, S, P);
      return vkr_gtao_reproject(ubo<vkr_gtao_reprojection>(st, 0, P), &depth, &pdepth, &ao, &pao, &out, st.stream);
    });
    create_program("deinterleave_depth", [=](LaunchState& st) {
      const char* P = "deinterleave_depth";
      vkr_img depth = tex(st, 0, T, P);
      auto layers = layers_of(st, 1, S, P);
      return vkr_deinterleave_depth(&depth, layers.data(), (uint32_t)layers.size(), push<vkr_deinterleave_push>(st, P), st.stream);
    });
    create_program("main_deinterleaved", [=](LaunchState& st) {
      const char* P = "main_deinterleaved";
      auto layers = layers_of(st, 0, T, P);
      vkr_img normal = tex(st, 2, T, P), out = tex(st, 3, S, P);
      return vkr_gtao_main_deinterleaved(layers.data(), (uint32_t)layers.size(), ubo<vkr_gtao_params>(st, 1, P), &normal, &out,
                                         push<vkr_gtao_deinterleaved_push>(st, P), st.stream);
    });
    // ---- ScreenSpaceTrace (row R2) ----
    create_program("screen_trace_main", [=](LaunchState& st) {
      const char* P = "screen_trace_main";
      vkr_img depth = tex(st, 0, T, P), normal = tex(st, 1, T, P), color = tex(st, 2, T, P), material = tex(st, 3, T, P), out = tex(st, 4, S, P);
      return vkr_screen_trace_main(&depth, &normal, &color, &material, &out, ubo<vkr_screen_trace_params>(st, 5, P), st.stream);
    });
    create_program("screen_trace_filter", [=](LaunchState& st) {
      const char* P = "screen_trace_filter";
      vkr_img raw = tex(st, 0, T, P), depth = tex(st, 1, T, P), out = tex(st, 2, S, P);
      return vkr_screen_trace_filter(&raw, &depth, &out, push<vkr_screen_trace_filter_push>(st, P), st.stream);
    });
    create_program("screen_trace_accumulate", [=](LaunchState& st) {
      const char* P = "screen_trace_accumulate";
      vkr_img depth = tex(st, 0, T, P), pdepth = tex(st, 1, T, P), cur = tex(st, 2, T, P), acc = tex(st, 3, S, P);
      return vkr_screen_trace_accumulate(&depth, &pdepth, &cur, &acc, push<vkr_screen_trace_accum_push>(st, P), st.stream);
    });
    // synthetic G-buffer "raster" program: attachments {albedo, normal, material, velocity, depth} or {depth}
    create_program("synthetic_gbuffer", [=](LaunchState& st) {
      const vkr_synth_params* p = ubo<vkr_synth_params>(st, 0, "synthetic_gbuffer");
      if (st.attachments.size() == 1) {
        vkr_img d = attachment(st, 0);
        return vkr_synth_gbuffer(&d, nullptr, nullptr, nullptr, nullptr, p, st.stream);
      }
      if (st.attachments.size() != 5) throw std::runtime_error{"synthetic_gbuffer: expects 4 colour attachments + depth"};
      vkr_img a = attachment(st, 0), n = attachment(st, 1), m = attachment(st, 2), v = attachment(st, 3), d = attachment(st, 4);
      return vkr_synth_gbuffer(&d, &n, &a, &m, &v, p, st.stream);
    });
  });
}

void BasePipeline::set_program(const std::string& name) {
  register_hot_path_programs();
  if (!gpu::has_program(name)) throw std::runtime_error{"Program not found"};
  program = name;
}
ComputePipeline create_compute_pipeline() { return ComputePipeline{}; }
ComputePipeline create_compute_pipeline(const char* name) { ComputePipeline p; p.set_program(name); return p; }
GraphicsPipeline create_graphics_pipeline() { return GraphicsPipeline{}; }

// ---- command context ---------------------------------------------------------------------------------------
void CmdContext::begin() {
  if (!staged_updates.empty()) {  // their async copies must have drained before the storage goes away
    (void)hipStreamSynchronize((hipStream_t)stream);
    staged_updates.clear();
  }
  ubo_pool.reset();
  sets.clear();
}
VkDescriptorSet CmdContext::allocate_set() {
  sets.emplace_back(new DescriptorSetObject{});
  return (VkDescriptorSet)sets.back().get();
}
void CmdContext::bind_pipeline(const ComputePipeline& p) {
  if (!p.has_program()) throw std::runtime_error{"Pipeline without program"};
  bound_program = p.program_name();
}
void CmdContext::bind_pipeline(const GraphicsPipeline& p) {
  if (!p.has_program()) throw std::runtime_error{"Pipeline without program"};
  bound_program = p.program_name();
}
void CmdContext::bind_sets(uint32_t first_set, const std::initializer_list<VkDescriptorSet>& s) {
  if (first_set > 1 || s.size() != 1) throw std::runtime_error{"Only descriptor sets 0 and 1 are used on this path"};
  (first_set == 0 ? state.set : state.set1) = (const DescriptorSetObject*)*s.begin();
}
CmdContext::~CmdContext() { device_free(state.scratch); device_free(state.workspace); }
void* LaunchState::require_workspace(uint64_t bytes) { return grow_only(workspace, workspace_bytes, bytes, stream); }
void* CmdContext::require_scratch(uint64_t bytes) { return grow_only(state.scratch, state.scratch_bytes, bytes, stream); }
void CmdContext::clear_color_attachments(float r, float g, float b, float a) {
  // the programs clear their own attachments: to 0, or (cubemap_probe, probe_renderer.cpp:121) to (100, 0, 0, 0)
  const bool zero = r == 0.f && g == 0.f && b == 0.f && a == 0.f, probe = r == 100.f && g == 0.f && b == 0.f && a == 0.f;
  if (!zero && !probe) throw std::runtime_error{"Only a clear to 0 or to (100, 0, 0, 0) is implemented on this path"};
  state.cleared_color = true;
  state.clear_color[0] = r; state.clear_color[1] = g; state.clear_color[2] = b; state.clear_color[3] = a;
}
void CmdContext::clear_depth_attachment(float depth) {
  if (depth != 1.f) throw std::runtime_error{"Only a depth clear to 1 is implemented on this path"};
  state.cleared_depth = true;
}
void CmdContext::bind_vertex_buffers(uint32_t first, const std::initializer_list<VkBuffer>& buffers, const std::initializer_list<uint64_t>& offsets) {
  if (first != 0 || buffers.size() != 1 || (offsets.size() && *offsets.begin() != 0)) throw std::runtime_error{"One vertex buffer at offset 0 is implemented on this path"};
  state.vertex_buffer = (Buffer*)*buffers.begin();
}
void CmdContext::bind_index_buffer(VkBuffer buffer, uint64_t offset, VkIndexType type) {
  if (offset != 0 || type != VK_INDEX_TYPE_UINT32) throw std::runtime_error{"A uint32 index buffer at offset 0 is implemented on this path"};
  state.index_buffer = (Buffer*)buffer;
}
void CmdContext::draw_indexed(uint32_t index_count, uint32_t instance_count, uint32_t first_index, int32_t vertex_offset, uint32_t) {
  if (instance_count != 1) throw std::runtime_error{"Instanced draws are not implemented on this path"};
  state.indexed_draws.push_back(LaunchState::IndexedDraw{push_data, index_count, first_index, vertex_offset});
}
void CmdContext::end_renderpass() {
  const bool cube_face = bound_program && *bound_program == "cubemap_probe" && !state.attachments.empty();  // cleared even without a draw
  const bool shadow_layer = bound_program && *bound_program == "default_shadow" && !state.attachments.empty();  // likewise
  if (!state.indexed_draws.empty() || cube_face || shadow_layer) {  // the recorded geometry is one pass of the bound raster program
    uint32_t triangles = 0;
    for (const auto& d : state.indexed_draws) triangles += d.index_count / 3u;
    if (shadow_layer) {
      require_scratch(vkr_default_shadow_scratch_bytes(state.fb_width, 1, triangles));
    } else if (cube_face) {
      // one face of a cube: the draws are kept with their attachments, the six faces are baked by one vkr_cubemap_probe when
      // the last one ends (host/probe_renderer.hpp)
      require_scratch(vkr_cubemap_probe_scratch_bytes(state.fb_width, triangles));
    } else {
      require_scratch(vkr_raster_scratch_bytes(state.fb_width, state.fb_height, triangles));
    }
    launch();
  }
  state.indexed_draws.clear();
  state.attachments.clear();
  state.set1 = nullptr;
  state.vertex_buffer = state.index_buffer = nullptr;
  state.cleared_color = state.cleared_depth = false;
}
void CmdContext::push_constants_compute(uint32_t offset, uint32_t size, const void* constants) {
  if (push_data.size() < offset + size) push_data.resize(offset + size);
  std::memcpy(push_data.data() + offset, constants, size);
}
void CmdContext::set_framebuffer(uint32_t width, uint32_t height, const std::initializer_list<ImageViewObject>& attachments) {
  state.fb_width = width; state.fb_height = height;
  state.attachments.assign(attachments.begin(), attachments.end());
}
void CmdContext::set_framebuffer(uint32_t width, uint32_t height, const std::vector<ImageViewObject>& attachments) {
  state.fb_width = width; state.fb_height = height;
  state.attachments = attachments;
}
void CmdContext::launch() {
  if (!bound_program) throw std::runtime_error{"No pipeline bound"};
  auto it = programs().find(*bound_program);
  if (it == programs().end()) throw std::runtime_error{"Program not found"};
  state.push = push_data.data();
  state.push_size = (uint32_t)push_data.size();
  state.stream = stream;
  int rc = it->second(state);
  push_data.clear();
  state.set = nullptr;
  check_status(rc, bound_program->c_str());
}
void CmdContext::dispatch(uint32_t x, uint32_t y, uint32_t z) {
  state.groups[0] = x; state.groups[1] = y; state.groups[2] = z;
  launch();
}
void CmdContext::dispatch_indirect(VkBuffer arguments) {
  if (!arguments) throw std::runtime_error{"dispatch_indirect: null argument buffer"};
  state.groups[0] = state.groups[1] = state.groups[2] = 0;
  state.indirect = (Buffer*)arguments;
  launch();
  state.indirect = nullptr;
}
void CmdContext::update_buffer_bytes(VkBuffer dst, uint64_t offset, const void* data, uint64_t size) {
  auto* b = (Buffer*)dst;
  if (!b || offset + size > b->get_size() || size > 65536) throw std::runtime_error{"update_buffer: range outside the buffer"};
  // like vkCmdUpdateBuffer the value is captured at record time: stage it in memory that outlives the copy
  staged_updates.emplace_back((const uint8_t*)data, (const uint8_t*)data + size);
  hipError_t e = hipMemcpyAsync((uint8_t*)b->device_ptr(stream) + offset, staged_updates.back().data(), size, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) throw std::runtime_error{std::string{"update_buffer failed: "} + hipGetErrorString(e)};
}
void CmdContext::draw(uint32_t vertex_count, uint32_t, uint32_t, uint32_t) {
  if (vertex_count != 3) throw std::runtime_error{"Only the full-screen triangle draw is implemented on this path"};
  launch();
}

}  // namespace gpu
