/* Declared double of <sensor_msgs/Imu.h> -- NOT ROS.  Included by the reference's scan registration, never used. */
#pragma once
