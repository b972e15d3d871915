// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY (see ros/ros.h).
#pragma once
namespace std_srvs {
struct Empty {
    struct Request {};
    struct Response {};
    Request request;
    Response response;
};
}  // namespace std_srvs
