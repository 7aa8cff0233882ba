// hip_device_block.h -- how a header-only C++ mirror stages the batch of one `_device` call: ONE device allocation and
// one host block of the same size and layout, one copy up and one copy down.
//
// The mirror writes its layout once, as a function of an msf::Carver& (carve.h) that returns a view: a small struct of
// typed pointers -- the inputs first, then `inputs_end = c.off`, then the outputs, usually as the call's public result
// struct.  place() runs that function on a null base to measure, on the device block and on the host block, so the same
// member of the two views is the same offset on the two sides and no offset is written down twice.  The mirror fills
// the inputs through the host view, upload()s, hands the device view's pointers to the call, download()s and reads the
// outputs through the host view.  Synchronous, like the mirrors: no stream.
#pragma once

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "carve.h"

namespace msf {

class DeviceBlock {
 public:
  DeviceBlock() = default;
  DeviceBlock(const DeviceBlock&) = delete;
  DeviceBlock& operator=(const DeviceBlock&) = delete;
  ~DeviceBlock() { release(); }

  // `layout`: View(Carver&), View having a member `size_t inputs_end`.  Frees what an earlier place() left, allocates
  // both blocks zeroed and fills *dev and *host.  false: hipMalloc or hipMemset failed; nothing is held then.
  template <class Layout, class View>
  bool place(Layout&& layout, View* dev, View* host) {
    release();
    Carver measure;
    layout(measure);
    const size_t room = measure.off ? measure.off : 256;
    host_.assign(room, 0);
    if (hipMalloc(&dev_, room) != hipSuccess) dev_ = nullptr;
    if (!dev_ || hipMemset(dev_, 0, room) != hipSuccess) {   // upload() orders the zeroing before the call
      release();
      return false;
    }
    Carver d{static_cast<uint8_t*>(dev_)}, h{host_.data()};
    *dev = layout(d);
    *host = layout(h);
    bytes_ = measure.off;
    inputs_ = host->inputs_end;
    return true;
  }

  // the inputs, [0, inputs_end), host -> device
  bool upload() { return dev_ && hipMemcpy(dev_, host_.data(), inputs_, hipMemcpyHostToDevice) == hipSuccess; }

  // the rest, [inputs_end, bytes), device -> host
  bool download() {
    return dev_ && hipMemcpy(host_.data() + inputs_, static_cast<uint8_t*>(dev_) + inputs_, bytes_ - inputs_,
                             hipMemcpyDeviceToHost) == hipSuccess;
  }

  size_t bytes() const { return bytes_; }   // what the layout measures: every piece rounded up to 256

 private:
  void release() {
    if (dev_) hipFree(dev_);
    dev_ = nullptr;
    bytes_ = inputs_ = 0;
  }

  void* dev_ = nullptr;
  std::vector<uint8_t> host_;
  size_t bytes_ = 0, inputs_ = 0;
};

}  // namespace msf
